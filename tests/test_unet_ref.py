"""tests/unet_ref.py against the reference's own UnetNeck (tests/golden/unet_neck.npz, written by tests/golden/gen_unet_golden.py
from the reference's unet.py on the CPU in fp32), bit for bit; and the state_dict layout of torchok_amd's UnetNeck against the
recorded one, so checkpoints interchange."""
import os

import numpy as np
import pytest
import torch

import torchok_amd as T
import unet_ref as U
from helpers import deterministic_state

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'unet_neck.npz'))
IN_CHANNELS, DECODER = GOLD['in_channels'].tolist(), tuple(GOLD['decoder_channels'].tolist())


def test_fixture_is_no_larger_than_the_largest_golden_file():
    d = os.path.join(os.path.dirname(__file__), 'golden')
    sizes = {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith('.npz')}
    assert sizes['unet_neck.npz'] <= max(v for f, v in sizes.items() if f != 'unet_neck.npz')
    assert sizes['unet_neck.npz'] <= 1 << 20


@pytest.fixture
def one_thread():
    """The fixture was written on one CPU thread (the convolution's weight-gradient reduction is split across threads, so its
    bits depend on the thread count); other tests of the suite change the count and leave it changed."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def test_restatement_reproduces_the_reference_bit_for_bit(one_thread):
    ref = U.UnetNeck(IN_CHANNELS, DECODER).train()
    assert list(ref.state_dict()) == [str(n) for n in GOLD['state_names']]
    ref.load_state_dict(deterministic_state(ref.state_dict(), int(GOLD['seed'])))
    h, w = GOLD['image_hw'].tolist()
    image = torch.zeros(2, 3, h, w)
    feats = [torch.from_numpy(GOLD[f'feat{i}']).requires_grad_(True) for i in range(len(IN_CHANNELS))]
    assert [tuple(f.shape[2:]) for f in feats] == [(h >> (i + 1), w >> (i + 1)) for i in range(5)] and feats[-1].shape[2:] == (2, 1)
    img, out = ref([image] + feats)
    assert img is image
    assert np.array_equal(out.detach().numpy(), GOLD['out'])
    out.backward(torch.from_numpy(GOLD['d_out']))
    for i, f in enumerate(feats):
        assert np.array_equal(f.grad.numpy(), GOLD[f'd_feat{i}']), i
    for n, p in ref.named_parameters():
        assert np.array_equal(p.grad.numpy(), GOLD[f'grad__{n}']), n
    for n, b in ref.named_buffers():
        assert np.array_equal(b.numpy(), GOLD[f'after__{n}']), n


def test_state_dict_has_the_recorded_names_and_shapes():
    neck = T.NECKS.get('UnetNeck')(IN_CHANNELS, decoder_channels=DECODER)
    sd = neck.state_dict()
    assert list(sd) == [str(n) for n in GOLD['state_names']]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in GOLD['state_shapes']]
    assert neck.out_channels == DECODER[-1] and tuple(neck.in_channels) == tuple(IN_CHANNELS)
    for i, blk in enumerate(neck.blocks):
        assert isinstance(blk.attention1, torch.nn.Identity) and isinstance(blk.attention2, torch.nn.Identity)
    # the default decoder on ResNet's encoder widths: unet.py:104-110 bookkeeping
    big = T.NECKS.get('UnetNeck')((64, 64, 128, 256, 512))
    assert [b.conv1.conv.in_channels for b in big.blocks] == [512 + 256, 512 + 128, 256 + 64, 128 + 64, 64]
    assert [b.conv2.conv.out_channels for b in big.blocks] == [512, 256, 128, 64, 64] and big.out_channels == 64
    assert big.center[0].conv.weight.shape == (512, 512, 3, 3)
