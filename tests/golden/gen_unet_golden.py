#!/usr/bin/env python
"""Generate tests/golden/unet_neck.npz from the REFERENCE's own UnetNeck (runs only where the reference checkout exists; the
fixture it writes is a small data file that travels).  The reference's necks/segmentation/unet.py, modules/blocks/scse.py and
modules/bricks/convbnact.py are loaded unmodified through the shim of gen_golden.py; the run is fp32 on the CPU in training
mode.  Parameters are deterministic_state(state_dict, seed), features and d(out) come from one seeded generator, so the fixture
holds everything a box without the reference needs: the features, the output, d(out), every input and parameter gradient and
the state_dict layout.  The run uses ONE CPU thread: the convolution's weight-gradient reduction is split across threads, so its
bits depend on the thread count; tests/test_unet_ref.py replays it on one thread as well."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from helpers import deterministic_state  # noqa: E402

IN_CHANNELS, DECODER, BATCH, IMAGE, SEED = [8, 8, 16, 24, 32], (32, 24, 16, 8, 8), 2, (64, 32), 97


def main(out_path=os.path.join(HERE, 'unet_neck.npz')):
    torch.set_num_threads(1)
    G.install_shim()
    REF = G.REF
    G._fake_pkg('torchok.models.modules', f'{REF}/models/modules')
    G._fake_pkg('torchok.models.modules.bricks', f'{REF}/models/modules/bricks')
    G._fake_pkg('torchok.models.modules.blocks', f'{REF}/models/modules/blocks')
    G._load('torchok.models.modules.bricks.convbnact', f'{REF}/models/modules/bricks/convbnact.py')
    G._load('torchok.models.modules.blocks.scse', f'{REF}/models/modules/blocks/scse.py')
    G._fake_pkg('torchok.models.necks', f'{REF}/models/necks')
    G._fake_pkg('torchok.models.necks.segmentation', f'{REF}/models/necks/segmentation')
    unet = G._load('torchok.models.necks.segmentation.unet', f'{REF}/models/necks/segmentation/unet.py')

    ref = unet.UnetNeck(in_channels=IN_CHANNELS, decoder_channels=DECODER).train()
    ref.load_state_dict(deterministic_state(ref.state_dict(), SEED))
    g = torch.Generator().manual_seed(SEED + 1)
    h, w = IMAGE
    image = torch.zeros(BATCH, 3, h, w)
    feats = [torch.randn(BATCH, c, h >> (i + 1), w >> (i + 1), generator=g).requires_grad_(True)
             for i, c in enumerate(IN_CHANNELS)]
    img, out = ref([image] + feats)
    assert img is image and tuple(out.shape) == (BATCH, DECODER[-1], h, w)
    d_out = torch.randn(out.shape, generator=g)
    out.backward(d_out)
    sd = ref.state_dict()
    arrays = {f'feat{i}': f.detach().numpy() for i, f in enumerate(feats)}
    arrays.update({f'd_feat{i}': f.grad.numpy() for i, f in enumerate(feats)})
    arrays.update({f'grad__{n}': p.grad.numpy() for n, p in ref.named_parameters()})
    arrays.update({f'after__{n}': b.numpy() for n, b in ref.named_buffers()})       # running statistics after the step
    np.savez_compressed(out_path, seed=SEED, in_channels=np.array(IN_CHANNELS), decoder_channels=np.array(DECODER),
                        image_hw=np.array(IMAGE), out=out.detach().numpy(), d_out=d_out.numpy(),
                        state_names=np.array(list(sd)), state_shapes=np.array([str(tuple(v.shape)) for v in sd.values()]),
                        **arrays)
    print(f'wrote {out_path}: {os.path.getsize(out_path)} bytes, {len(sd)} state_dict entries')


if __name__ == '__main__':
    main()
