"""The plain-torch ResNeXt the build is compared with, composed from the oracle's own pieces: oracle.timm_min.Bottleneck already
passes groups=cardinality to conv2 and computes width = floor(planes * base_width / 64) * cardinality, and
oracle.torchok_ref.ResNet / make_blocks hand base_width through to the block.  The only thing added is a Bottleneck subclass
that fixes the cardinality (the oracle's ResNet has no such argument), and the constructors under the reference's names in the
runtime dict oracle.torchok_ref.BACKBONES, so that oracle.torchok_ref.ClassificationModel builds them."""
import oracle.timm_min as TM
import oracle.torchok_ref as R


def _bottleneck(cardinality):
    class GroupedBottleneck(TM.Bottleneck):
        def __init__(self, inplanes, planes, stride=1, downsample=None, **kw):
            super().__init__(inplanes, planes, stride, downsample, cardinality=cardinality, **kw)
    GroupedBottleneck.__name__ = f'Bottleneck{cardinality}'
    return GroupedBottleneck


_B32, _B64 = _bottleneck(32), _bottleneck(64)
_D = dict(stem_width=32, stem_type='deep', avg_down=True)

# name -> (block, layers, base_width, further ResNet arguments): the arguments of reference resnet.py:787-993
SPECS = {
    'resnext50_32x4d': (_B32, [3, 4, 6, 3], 4, {}),
    'resnext50d_32x4d': (_B32, [3, 4, 6, 3], 4, _D),
    'resnext101_32x4d': (_B32, [3, 4, 23, 3], 4, {}),
    'resnext101_32x8d': (_B32, [3, 4, 23, 3], 8, {}),
    'resnext101_64x4d': (_B64, [3, 4, 23, 3], 4, {}),
}
TWINS = {'tv_resnext50_32x4d': 'resnext50_32x4d', 'ig_resnext101_32x8d': 'resnext101_32x8d',
         'ssl_resnext50_32x4d': 'resnext50_32x4d', 'ssl_resnext101_32x4d': 'resnext101_32x4d',
         'ssl_resnext101_32x8d': 'resnext101_32x8d', 'swsl_resnext50_32x4d': 'resnext50_32x4d',
         'swsl_resnext101_32x4d': 'resnext101_32x4d', 'swsl_resnext101_32x8d': 'resnext101_32x8d'}
DEFAULT_PRETRAINED = [n for n in TWINS if n.split('_')[0] in ('ig', 'ssl', 'swsl')]
NAMES = list(SPECS) + list(TWINS)
NOT_BUILT = ['ig_resnext101_32x16d', 'ig_resnext101_32x32d', 'ig_resnext101_32x48d', 'ssl_resnext101_32x16d',
             'swsl_resnext101_32x16d']          # group widths up to 384: no kernel, no entry point


def _ctor(name):
    block, layers, base_width, extra = SPECS[name]

    def make(**kw):
        return R.ResNet(block, layers, base_width=base_width, **extra, **kw)
    make.__name__ = name
    return make


for _n in SPECS:
    R.BACKBONES.setdefault(_n, _ctor(_n))
for _n, _of in TWINS.items():
    R.BACKBONES.setdefault(_n, R.BACKBONES[_of])
