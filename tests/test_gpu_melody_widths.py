"""-m gpu: melody_size 12 and 16 (csrc/notes.hip at W = 12 / 16) on an MI355X against the oracle: one-clip plans at two
shapes, batched plans up to the 64-clip regime, the reference's Python surface, and the eight- and twelve-wave buckets of the
applier's backward (C = 9, 17) with melody_size 8 beside them as a control."""
import pytest
import torch

import parity_cases as pc
from oracle import style_oracle as so
from tools.synth import synth_clip
from simutil import rel
from test_host_surface import build_model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FULL = pc.FULL


@pytest.fixture(scope='module')
def native():
    from style import _native as nat
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


@pytest.mark.parametrize('C,R,T', [(2, 8, 4), (4, 16, 4)])
@pytest.mark.parametrize('W', [12, 16])
def test_note_kernels_match_the_oracle(native, W, C, R, T):
    e, worst = pc.oracle_case(native, DEV, dict(FULL, melody=W), C, R, T, True, check_bitwise=True)
    print(f'melody {W} C{C} R{R} T{T}: all-gradient rel-L2 {e:.3g} worst tensor {worst:.3g}')


def test_batched_plan_equals_sequential_iterations(native):
    pc.batch_case(native, DEV, dict(FULL, melody=16), 2, 4, 2, True, 8)


def test_64_clip_plan_at_the_bench_shape(native):
    # the regime of the --full bench line: 64 x 64 GEMM tiling, conv.hip / lin.hip kernels; every clip against the oracle and
    # bitwise against the one-clip plan
    pc.batch_case(native, DEV, dict(FULL, melody=16), 4, 16, 4, True, 64)


def test_melody16_model_trains_like_the_oracle():
    """The reference's surface at melody_size=16: the constructor accepts it, and two train-model.py loop bodies (fused
    train_iteration + FusedAdam.step()) give the oracle's loss leaves on the same seeded clips and parameters."""
    from style import _native as nat
    from style.optim import FusedAdam
    model = build_model(dict(FULL, melody=16), seed=7)
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


def test_melody16_inference_matches_the_oracle():
    """extract_style -> predict_song_info -> apply_style -> hard_output at melody_size=16 (style of song B, pitched only, on
    melody + rhythm of song A) against the oracle; hard_output exact on the oracle's own prediction."""
    import style.model as m
    model = build_model(dict(FULL, melody=16), seed=7)
    named = {n: p.detach().clone() for n, p in model.named_parameters()}
    model = model.to(DEV)
    C, R, T = 2, 4, 2
    ca, cb = (synth_clip(k, C, R, T, True) for k in (50, 51))
    a, b = ({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()} for c in (ca, cb))
    with torch.no_grad():
        style_a, melody_a, rhythm_a = model.extract_style(a['mode'], a['bpm'], a['pitched'], a['instruments_features'], a['unpitched'])
        style_b, _, _ = model.extract_style(b['mode'], b['bpm'], b['pitched'], b['instruments_features'], None)
        ip, mp, bp = model.predict_song_info(style_b, rhythm_a)
        xp, xu = model.apply_style(style_b, melody_a, rhythm_a, b['instruments_features'][:, :1], True)
        r_style_a, r_melody_a, r_rhythm_a = so.extract_style(named, ca['mode'], ca['bpm'], ca['pitched'], ca['instruments_features'], ca['unpitched'])
        r_style_b, _, _ = so.extract_style(named, cb['mode'], cb['bpm'], cb['pitched'], cb['instruments_features'], None)
        P = so.Params(named)
        r_ip, r_mp, r_bp = so.song_info(P.sub('song_info_model'), r_style_b, r_rhythm_a)
        r_xp = so.pitched_style_applier(P.sub('pitched_style_applier'), r_style_b, r_melody_a, r_rhythm_a, cb['instruments_features'][:, :1])
        r_xu = so.unpitched_style_applier(P.sub('unpitched_style_applier'), r_style_b, r_rhythm_a)
    assert melody_a.shape == (1, R, T, 10, 56, 16)
    for got, ref, key in ((style_a, r_style_a, 'style_a'), (style_b, r_style_b, 'style_b'), (melody_a, r_melody_a, 'melody_a'),
                          (rhythm_a, r_rhythm_a, 'rhythm_a'), (ip, r_ip, 'instruments'), (mp, r_mp, 'mode'), (bp, r_bp, 'bpm'),
                          (xp, r_xp, 'pitched'), (xu, r_xu, 'unpitched')):
        assert tuple(got.shape) == tuple(ref.shape), key
        assert rel(got.cpu().numpy(), ref.numpy()) < pc.TOL, key
    for ref in (r_xp, r_xu):
        x = ref.clone().to(DEV)
        want_in = ref.clone()
        want = so.hard_output(want_in)
        y = m.hard_output(x)
        assert torch.equal(y.cpu(), want) and torch.equal(x.cpu(), want_in)


# the 8-wave (C = 9 .. 16) and the 12-wave (C = 17 .. 24) bucket of psa_bwd2; melody 8 is the control: a failure there at
# the same channel count is a defect the parent already has, not one of the wide instantiations
@pytest.mark.parametrize('C', [9, 17])
@pytest.mark.parametrize('W', [8, 16])
def test_many_channels(native, W, C):
    e, worst = pc.oracle_case(native, DEV, dict(FULL, melody=W), C, 2, 2, True, check_bitwise=True)
    print(f'melody {W} C{C}: all-gradient rel-L2 {e:.3g} worst tensor {worst:.3g}')
