"""Shared cases and arbiters of the guarded optimizer step (mst_adam_step_guarded, mst_grad_norm, mst_grad_norms), used by the
CPU-interpreter tests and the GPU tests alike: everything here works on torch tensors of any device and a ctypes binding of the
C ABI (`lib`).  The arbiters are numpy on the host; the bitwise arbiter of a clipped step is the UNGUARDED entry point of the
same library on host-scaled gradients."""
import numpy as np
import torch

SIZES = (1, 3, 255, 256, 1025, 4099, 70001)
HYPER = (.01, .9, .999, 1e-8, 200, .9)          # lr0, beta1, beta2, eps, step_size, gamma
ERR_ARG = -1
INF = float('inf')


def mixed(n, seed):
    """n fp32 values of mixed sign and magnitude, 1e-20 to 1e15."""
    r = np.random.RandomState(seed)
    return (r.choice([-1., 1.], n) * 10. ** r.uniform(-20, 15, n)).astype(np.float32)


def effective(g, g2=None):
    """The effective gradient as the kernels form it: g + g2 in fp32."""
    return g if g2 is None else (g.astype(np.float32) + g2.astype(np.float32)).astype(np.float32)


def arbiter_norm(g, g2=None):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.float32(np.sqrt(np.sum(effective(g, g2).astype(np.float64) ** 2)))


def ulps(a, b):
    """Distance of two finite fp32 values in units in the last place."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))


def coef_formula(norm, max_norm):
    """clip_grad_norm_'s coefficient in fp32, in torch's order of evaluation: reciprocal, then multiply, clamped at 1."""
    c = np.float32(max_norm) * (np.float32(1) / (np.float32(norm) + np.float32(1e-6)))
    return c if c < np.float32(1) else np.float32(1)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Bufs:
    """params / grads / moments / state / guard / scratch of one optimizer on `device`.  lead = 1 puts every float buffer one
    float behind a 16-byte boundary (the kernels' ragged head)."""

    def __init__(self, lib, n, device='cpu', two=False, lead=0, seed=0):
        self.lib, self.n, self.device, self.lead = lib, n, torch.device(device), lead
        r = np.random.RandomState(seed)
        mk = lambda a: self._put(torch.from_numpy(np.asarray(a, dtype=np.float32)))
        self.p = mk(r.uniform(-1, 1, n))
        self.g = mk(np.zeros(n))
        self.g2 = mk(np.zeros(n)) if two else None
        self.m, self.v = mk(np.zeros(n)), mk(np.zeros(n))
        self.state = torch.zeros(4, device=self.device)
        self.guard = torch.zeros(8, device=self.device)
        nbytes = lib.mst_grad_guard_scratch_bytes(n)
        assert nbytes > 0 and nbytes % 8 == 0
        self.scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)

    def _put(self, host):
        buf = torch.zeros(host.numel() + 8, dtype=torch.float32, device=self.device)
        assert buf.data_ptr() % 16 == 0
        out = buf[self.lead:self.lead + host.numel()]
        out.copy_(host)
        return out

    def clone(self):
        c = Bufs.__new__(Bufs)
        c.lib, c.n, c.device, c.lead = self.lib, self.n, self.device, self.lead
        for k in ('p', 'g', 'g2', 'm', 'v'):
            t = getattr(self, k)
            setattr(c, k, None if t is None else c._put(t.detach().cpu()))
        c.state, c.guard, c.scratch = self.state.clone(), self.guard.clone(), self.scratch.clone()
        return c

    def set_grads(self, g, g2=None):
        self.g.copy_(torch.from_numpy(np.asarray(g, dtype=np.float32)))
        if self.g2 is not None:
            self.g2.copy_(torch.from_numpy(np.asarray(g2 if g2 is not None else np.zeros(self.n), dtype=np.float32)))

    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == 'cuda' else None

    def ptr(self, t):
        return None if t is None else t.data_ptr()

    def plain(self, zero_grad=1):
        P = self.ptr
        if self.g2 is None:
            return self.lib.mst_adam_step(P(self.p), P(self.g), P(self.m), P(self.v), self.n, P(self.state), *HYPER, zero_grad, self.stream())
        return self.lib.mst_adam_step2(P(self.p), P(self.g), P(self.g2), P(self.m), P(self.v), self.n, P(self.state), *HYPER, zero_grad,
                                       self.stream())

    def guarded(self, max_norm, skip_nonfinite=0, zero_grad=1):
        P = self.ptr
        return self.lib.mst_adam_step_guarded(P(self.p), P(self.g), P(self.g2), P(self.m), P(self.v), self.n, P(self.state), P(self.guard),
                                              P(self.scratch), *HYPER, max_norm, skip_nonfinite, zero_grad, self.stream())

    def norm(self):
        out = torch.zeros(1, device=self.device)
        rc = self.lib.mst_grad_norm(self.ptr(self.g), self.ptr(self.g2), self.n, self.ptr(self.scratch), out.data_ptr(), self.stream())
        assert rc == 0, rc
        return np.float32(out.cpu().numpy()[0])

    def same_optimizer(self, other):
        return all(same_bits(getattr(self, k), getattr(other, k)) for k in ('p', 'm', 'v', 'state'))


def nonfinite_cases(n, seed=7):
    """(name, g, g2 or None) — gradients whose effective fp32 norm is inf or NaN."""
    base, other = mixed(n, seed) * np.float32(1e-15), mixed(n, seed + 1) * np.float32(1e-15)
    out = []
    g = base.copy(); g[-1] = np.nan
    out.append(('nan_last', g, None))
    g = base.copy(); g[0] = np.inf
    out.append(('inf_first', g, None))
    g2 = other.copy(); g2[n // 2] = np.nan
    out.append(('nan_in_grads2', base.copy(), g2))
    g, g2 = base.copy(), other.copy(); g[n // 3], g2[n // 3] = np.inf, -np.inf
    out.append(('inf_minus_inf', g, g2))
    g = base.copy(); g[:2] = np.float32(3e38)          # every element finite, the sum of squares finite in double, its root beyond fp32
    out.append(('norm_overflows_fp32', g, None))
    return out


def check_clip_is_scale_then_step(lib, n, device, two, steps=3, seed=11):
    """Guarded steps with max_norm = half the arbiter norm against the unguarded entry point on host-scaled gradients."""
    a = Bufs(lib, n, device, two=two, seed=seed)
    b = a.clone()
    for k in range(steps):
        g, g2 = mixed(n, seed + 10 * k), (mixed(n, seed + 10 * k + 1) if two else None)
        want_norm = arbiter_norm(g, g2)
        max_norm = float(want_norm) / 2
        a.set_grads(g, g2)
        assert a.guarded(max_norm) == 0
        guard = a.guard.cpu().numpy()
        assert ulps(guard[0], want_norm) <= 1, (guard[0], want_norm)
        assert guard[1] < 1 and guard[2] == 0 and guard[4] == k + 1 and guard[3] == 0, guard
        assert ulps(guard[1], coef_formula(guard[0], max_norm)) <= 1, (guard[1], coef_formula(guard[0], max_norm))
        assert ulps(guard[5], max(arbiter_norm(mixed(n, seed + 10 * j), mixed(n, seed + 10 * j + 1) if two else None)
                                  for j in range(k + 1))) <= 1
        b.set_grads(effective(g, g2) * np.float32(guard[1]))          # fp32 product, rounded once
        assert b.plain() == 0
        assert a.same_optimizer(b), (n, two, k)
        assert not a.g.any() and (a.g2 is None or not a.g2.any())
    assert float(a.state[0]) == steps


def check_skip(lib, n, device, name, g, g2, zero_grad):
    two = g2 is not None
    good1, good2 = mixed(n, 21) * np.float32(1e-12), mixed(n, 22) * np.float32(1e-12)
    a = Bufs(lib, n, device, two=two, seed=5)
    a.set_grads(good1)
    assert a.guarded(1., 1) == 0                                    # a good, clipped step first: non-zero moments, t = 1
    assert float(a.guard[2]) == 0 and float(a.state[0]) == 1
    ref = a.clone()                                                  # the run that never sees the bad gradient
    before = a.clone()
    a.set_grads(g, g2)
    assert a.guarded(1., 1, zero_grad) == 0
    assert a.same_optimizer(before), name                            # p, m, v and state bit-unchanged
    guard = a.guard.cpu().numpy()
    assert guard[2] == 1 and guard[1] == 0 and guard[3] == 1 and not np.isfinite(guard[0]), (name, guard)
    assert guard[4] == before.guard[4].item() and guard[5] == before.guard[5].item()
    if zero_grad:
        assert not a.g.any() and (a.g2 is None or not a.g2.any())
    else:
        before.set_grads(g, g2)
        assert same_bits(a.g, before.g) and (a.g2 is None or same_bits(a.g2, before.g2))
    for x in (a, ref):                                               # the next good step is step t + 1 = 2 of the clean run
        x.set_grads(good2)
        assert x.guarded(1., 1) == 0
    assert a.same_optimizer(ref) and float(a.state[0]) == 2, name
    assert float(a.guard[3]) == 1 and float(a.guard[2]) == 0
    # skip_nonfinite = 0: the unguarded step on the same data (coef = 1), NaNs and all
    c = Bufs(lib, n, device, two=two, seed=5)
    d = c.clone()
    for x in (c, d):
        x.set_grads(g, g2)
    assert c.guarded(1., 0, zero_grad) == 0 and d.plain(zero_grad) == 0
    assert c.same_optimizer(d) and same_bits(c.g, d.g), name
    assert float(c.guard[1]) == 1 and float(c.guard[2]) == 0 and float(c.guard[3]) == 0
