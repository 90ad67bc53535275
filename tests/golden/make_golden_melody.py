"""Generate tests/golden/small_melody16.npz by RUNNING the reference at melody_size 16 (build container only).

    PYTHONPATH=<reference checkout>:<this repository> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_melody.py

The `small_case` recipe of make_golden.py (the reference's `style.model` imported unmodified, seed 7, synthetic clips 0 and 1
of tools/synth.py with percussion, one Adam + StepLR step after the second clip) at dict(SMALL, melody=16); the widths are
stored in the file.  The post-Adam parameters `p1/*` are left out to keep the file no larger than the largest fixture
already here (Adam does not depend on a width; the two existing small fixtures pin it).  Data only; nothing of the
reference's source travels.
"""
import os

import numpy as np
import torch

import make_golden as mg                     # imports the reference and checks where it came from

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = dict(mg.SMALL, melody=16)


def melody_case(name, widths, unpitched=True):
    C, R, T = 2, 3, 2
    model = mg.build(widths, seed=7)
    out = dict(widths=np.array([widths[k] for k in ('beat', 'bar', 'nrf', 'style', 'melody', 'rhythm')]),
               crt=np.array([C, R, T]), unpitched=np.array(int(unpitched)), density=np.array(0.05))
    for n, p in model.named_parameters():
        out['p0/' + n] = p.detach().numpy().copy()
    model.zero_grad()
    l0 = mg.iteration(model, mg.synth_clip(0, C, R, T, unpitched, density=0.05), capture=out)
    for n, p in model.named_parameters():
        out['g0/' + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    l1 = mg.iteration(model, mg.synth_clip(1, C, R, T, unpitched, density=0.05))
    for k, v in l0.items():
        out['loss0/' + k] = np.array(v)
    for k, v in l1.items():
        out['loss1/' + k] = np.array(v)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print(name, 'total0', l0['total'], 'total1', l1['total'], len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    melody_case('small_melody16', WIDTHS)
