"""-m gpu: LSTM hidden sizes above 256 (csrc/lstm.hip wide flavour, up to 1024) on an MI355X against the oracle, in batched
plans, and through the reference's Python surface (style.model) for a wide style width."""
import pytest
import torch

import parity_cases as pc
from tools.synth import synth_clip
from test_host_surface import build_model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FULL = pc.FULL


@pytest.fixture(scope='module')
def native():
    from style import _native as nat
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


@pytest.mark.parametrize('w,C,R,T', [
    (dict(FULL, style=512), 2, 8, 4),         # style encoder H 320
    (dict(FULL, bar=640), 2, 8, 4),           # bidirectional bars LSTMs 320, style encoder 448
    (dict(FULL, beat=320), 4, 4, 2),          # beats LSTMs 320 over C * R = 16 (pitched) and R = 4 (unpitched) sequences
    (dict(FULL, style=1920), 2, 8, 4),        # style encoder H 1024
])
def test_wide_lstms_match_the_oracle(native, w, C, R, T):
    e, worst = pc.oracle_case(native, DEV, w, C, R, T, True, check_bitwise=True)
    print(w, 'all-gradient rel-L2', e, 'worst tensor', worst)


def test_batched_wide_plan_equals_sequential_iterations(native):
    pc.batch_case(native, DEV, dict(FULL, style=512), 2, 4, 2, True, 8)


def test_wide_style_model_trains_like_the_oracle():
    """The reference's surface at style_size=512: the constructor accepts it, and two train-model.py loop bodies (fused
    train_iteration + FusedAdam.step()) give the oracle's loss leaves on the same seeded clips and parameters."""
    from oracle import style_oracle as so
    from style import _native as nat
    from style.optim import FusedAdam
    model = build_model(dict(FULL, style=512), seed=7)
    named = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters()}
    model = model.to(DEV)
    opt = FusedAdam(model)
    ref_opt = so.Adam(named.values())
    C, R, T = 2, 8, 4
    for it in range(2):
        clip = synth_clip(30 + it, C, R, T, True)
        d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in clip.items()}
        got = model.train_iteration(d['mode'], d['bpm'], d['pitched'], d['instruments_features'], d['unpitched'],
                                    d['used_instruments'], d['bpm_int'])
        torch.cuda.synchronize()                  # FusedAdam alternates the calls between two side-stream lanes
        got = got.cpu()
        _, ref = so.iteration(named, clip)
        for i, k in enumerate(nat.LOSS_KEYS):
            if k in ref:
                assert abs(float(got[i]) - ref[k]) < 3e-4, (it, k, float(got[i]), ref[k])
        opt.step()
        ref_opt.step()
