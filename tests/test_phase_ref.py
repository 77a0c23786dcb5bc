"""The identity the dilated stages rest on, held against torch itself in fp64 on integers (every value exact): a 3x3 / stride-1
convolution with dilation d and padding d equals the plain 3x3 / padding-1 convolution applied to each of the d x d phase images
x[:, a::d, b::d] when h and w are multiples of d — dense, grouped, and with d = 4 reached as two nested splits by 2.  The split
and merge used here are the torch statements of tok_phase_split / tok_phase_merge (include/tok.h), which the kernel contract test
and the stand-in of tests/test_dilated_resnet.py are compared with."""
import pytest
import torch
import torch.nn.functional as F


def split(x, d):
    """(n, c, h, w) -> (n * d * d, c, h / d, w / d): image (i, a, b) = x[i, :, a::d, b::d] at index (i * d + a) * d + b"""
    n, c, h, w = x.shape
    return x.view(n, c, h // d, d, w // d, d).permute(0, 3, 5, 1, 2, 4).reshape(n * d * d, c, h // d, w // d)


def merge(xs, d):
    nb, c, hq, wq = xs.shape
    n = nb // (d * d)
    return xs.view(n, d, d, c, hq, wq).permute(0, 3, 4, 1, 5, 2).reshape(n, c, hq * d, wq * d)


def _ints(shape, seed):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize('d', [2, 4])
def test_split_is_the_strided_slices_and_merge_its_inverse(d):
    x = _ints((2, 3, 2 * d, 3 * d), 1)
    xs = split(x, d)
    for i in range(2):
        for a in range(d):
            for b in range(d):
                assert torch.equal(xs[(i * d + a) * d + b], x[i, :, a::d, b::d])
    assert torch.equal(merge(xs, d), x)
    assert torch.equal(split(merge(xs, d), d), xs)


@pytest.mark.parametrize('groups', [1, 4, 8])
@pytest.mark.parametrize('d', [2, 4])
def test_dilated_conv_is_the_plain_conv_on_the_phase_images(d, groups):
    x = _ints((2, 16, 3 * d, 2 * d), 10 * d + groups).requires_grad_(True)
    w = _ints((16, 16 // groups, 3, 3), 20 * d + groups).requires_grad_(True)
    gy = _ints((2, 16, 3 * d, 2 * d), 30 * d + groups)
    want = F.conv2d(x, w, padding=d, dilation=d, groups=groups)
    dx, dw = torch.autograd.grad(want, (x, w), gy)
    got = merge(F.conv2d(split(x, d), w, padding=1, groups=groups), d)
    dx2, dw2 = torch.autograd.grad(got, (x, w), gy)
    assert torch.equal(got, want) and torch.equal(dx2, dx) and torch.equal(dw2, dw)


@pytest.mark.parametrize('groups', [1, 4])
def test_dilation_4_as_two_nested_splits_by_2(groups):
    x = _ints((2, 8, 8, 12), 41 + groups)
    w = _ints((8, 8 // groups, 3, 3), 42 + groups)
    want = F.conv2d(x, w, padding=4, dilation=4, groups=groups)
    xs = split(split(x, 2), 2)
    assert torch.equal(merge(merge(F.conv2d(xs, w, padding=1, groups=groups), 2), 2), want)
    # the order of the nested index: the INNER split holds the higher bit of the phase, image
    # ((i * 2 + a1) * 2 + b1) * 4 + a2 * 2 + b2 holds the pixels Y = 4y + 2 * a2 + a1, X = 4x + 2 * b2 + b1
    for i in range(2):
        for a1 in range(2):
            for b1 in range(2):
                for a2 in range(2):
                    for b2 in range(2):
                        img = ((i * 2 + a1) * 2 + b1) * 4 + a2 * 2 + b2
                        assert torch.equal(xs[img], x[i, :, 2 * a2 + a1::4, 2 * b2 + b1::4])
    # ... every image is a phase image of dilation 4, but not in the order of one split by 4
    assert not torch.equal(xs, split(x, 4))
    assert sorted(map(lambda t: t.flatten().tolist(), xs)) == sorted(map(lambda t: t.flatten().tolist(), split(x, 4)))


def test_a_map_that_is_not_divisible_has_no_such_identity():
    """h % d != 0: the phase images differ in size, which is why the engine refuses such a map instead of padding it"""
    x = _ints((1, 1, 5, 4), 7)
    assert x[0, :, 0::2].shape != x[0, :, 1::2].shape
