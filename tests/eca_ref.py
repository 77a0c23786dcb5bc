"""References of the ECA residual unit (csrc/eca.hip, engine.functional.eca_residual) and of the ECA-ResNets.

The semantics are those of [timm 0.6.13] layers/eca.py EcaModule and resnet.py Bottleneck.forward (`self.se` sits behind the last
BatchNorm and in front of the residual add and the last activation).  timm is not installed next to this repository, so they are
RECALLED FROM UPSTREAM, not copied from a checked-out source (as SURVEY.md App. A says of the other timm pieces):

    k(C) = max(t if t odd else t + 1, 3),  t = int(|log2(C) + 1| / 2)
    m = mean_hw(z);  a = Conv1d(1, 1, k, padding=k // 2, bias=False)(m over the channel axis);  g = sigmoid(a)
    out = relu(z * g + shortcut)

Here: the fp64 unit with its closed-form backward, k(C), a Bottleneck of the oracle with that module, and the nine entry points
of the reference (resnet.py:1008-1101) in the runtime dict oracle.torchok_ref.BACKBONES so that
oracle.torchok_ref.ClassificationModel builds them."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle.timm_min as TM
import oracle.torchok_ref as R


def eca_k(channels, gamma=2, beta=1):
    t = int(abs(math.log(channels, 2) + beta) / gamma)
    return max(t if t % 2 else t + 1, 3)


# ---- the unit in fp64 ------------------------------------------------------------------------------------------------------
def _window(v, w):
    """[n][c] -> sum_j w[j] v[n][c + j - k//2], zero outside: nn.Conv1d(1, 1, k, padding=k // 2, bias=False) over the channels"""
    k = w.numel()
    return F.conv1d(v.unsqueeze(1), w.view(1, 1, k), padding=k // 2).squeeze(1)


def eca_residual_ref(z, shortcut, w):
    """z, shortcut [n][hw][c], w [k] -> (out, mean, gate) in fp64, nothing rounded"""
    z, shortcut, w = z.double(), shortcut.double(), w.double()
    mean = z.mean(1)
    gate = torch.sigmoid(_window(mean, w))
    return torch.relu(z * gate.unsqueeze(1) + shortcut), mean, gate


def eca_residual_bwd_ref(dout, out, z, w, mean, gate):
    """The closed-form backward, with the mask read from `out` (the stored output).  -> dict(dw, dz, dshort, dg, da, dmean)"""
    dout, z, w, mean, gate = dout.double(), z.double(), w.double(), mean.double(), gate.double()
    k, hw = w.numel(), z.shape[1]
    dm = dout * (out > 0)
    dg = (dm * z).sum(1)
    da = dg * gate * (1 - gate)
    mp = F.pad(mean, (k // 2, k // 2))
    c = mean.shape[1]
    dw = torch.stack([(da * mp[:, j:j + c]).sum() for j in range(k)])
    dmean = _window(da, w.flip(0))                   # sum_j w[j] da[c - j + k//2]
    dz = dm * gate.unsqueeze(1) + dmean.unsqueeze(1) / hw
    return dict(dw=dw, dz=dz, dshort=dm, dg=dg, da=da, dmean=dmean)


# ---- the networks ----------------------------------------------------------------------------------------------------------
class EcaModule(nn.Module):
    def __init__(self, channels):
        super().__init__()
        k = eca_k(channels)
        self.conv = nn.Conv1d(1, 1, kernel_size=k, padding=k // 2, bias=False)

    def forward(self, x):
        y = x.mean((2, 3)).view(x.shape[0], 1, -1)
        y = self.conv(y).view(x.shape[0], -1, 1, 1).sigmoid()
        return x * y.expand_as(x)


def _bottleneck(cardinality):
    class EcaBottleneck(TM.Bottleneck):
        def __init__(self, inplanes, planes, stride=1, downsample=None, **kw):
            super().__init__(inplanes, planes, stride, downsample, cardinality=cardinality, **kw)
            # `se` is assigned behind bn3 and in front of act3 / downsample: the state_dict order of the reference
            tail = [(n, self._modules.pop(n)) for n in ('act3', 'downsample') if n in self._modules]
            self.se = EcaModule(planes * self.expansion)
            for n, m in tail:
                self._modules[n] = m

        def forward(self, x):
            shortcut = x
            x = self.act1(self.bn1(self.conv1(x)))
            x = self.act2(self.bn2(self.conv2(x)))
            x = self.se(self.bn3(self.conv3(x)))
            if self.downsample is not None:
                shortcut = self.downsample(shortcut)
            return self.act3(x + shortcut)
    EcaBottleneck.__name__ = f'EcaBottleneck{cardinality}'
    return EcaBottleneck


EcaBottleneck, _E32 = _bottleneck(1), _bottleneck(32)
_D = dict(stem_width=32, stem_type='deep', avg_down=True)
_T = dict(stem_width=32, stem_type='deep_tiered', avg_down=True)

# name -> (block, layers, base_width, further ResNet arguments): the arguments of reference resnet.py:1008-1101
SPECS = {
    'ecaresnet26t': (EcaBottleneck, [2, 2, 2, 2], 64, _T),
    'ecaresnet50d': (EcaBottleneck, [3, 4, 6, 3], 64, _D),
    'ecaresnet50t': (EcaBottleneck, [3, 4, 6, 3], 64, _T),
    'ecaresnetlight': (EcaBottleneck, [1, 1, 11, 3], 64, dict(avg_down=True)),     # (stem_width=32 without a deep stem: unused)
    'ecaresnet101d': (EcaBottleneck, [3, 4, 23, 3], 64, _D),
    'ecaresnet200d': (EcaBottleneck, [3, 24, 36, 3], 64, _D),
    'ecaresnet269d': (EcaBottleneck, [3, 30, 48, 8], 64, _D),
    'ecaresnext26t_32x4d': (_E32, [2, 2, 2, 2], 4, _T),
    'ecaresnext50t_32x4d': (_E32, [2, 2, 2, 2], 4, _T),        # the reference gives it the layers of the 26t (resnet.py:1099)
}
NAMES = list(SPECS)


def _ctor(name):
    block, layers, base_width, extra = SPECS[name]

    def make(**kw):
        return R.ResNet(block, layers, base_width=base_width, **extra, **kw)
    make.__name__ = name
    return make


for _n in SPECS:
    R.BACKBONES.setdefault(_n, _ctor(_n))
