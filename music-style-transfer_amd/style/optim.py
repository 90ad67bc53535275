"""Fused Adam + StepLR over the model's flat parameter buffer (train-model.py:89-90,151-154).

`torch.optim.Adam(model.parameters())` keeps working on this package's model (the parameters are
ordinary nn.Parameters whose .grad aliases the flat gradient buffer); this class is the HIP
equivalent of `optimizer.step(); optimizer.zero_grad(); scheduler.step()` in one launch, with
the step counter and the per-step scalars kept on the device so that it is graph-replayable.
For data parallelism pass `process_group`: gradients are all-reduced with SUM (RCCL) — the
reference accumulates gradients without averaging (train-model.py:126,151-153).

Opt-in guard (`max_grad_norm`, `skip_nonfinite`): the global L2 norm of the summed gradient is taken on the device, the
gradient is clipped to `max_grad_norm` and a step whose norm is inf / NaN is skipped, all inside the step's launches
(mst_adam_step_guarded: one launch more, still no host synchronisation, still graph-replayable).
"""
import math

import torch

from style import _native


class FusedAdam:
    GUARD_KEYS = ('norm', 'coef', 'skipped', 'steps_skipped', 'steps_clipped', 'largest_norm')     # guard record words 0..5

    def __init__(self, model, lr=.01, betas=(.9, .999), eps=1e-8, step_size=200, gamma=.9, process_group=None,
                 max_grad_norm=None, skip_nonfinite=False):
        model._sync_flat()
        self.model = model
        self.lr, self.betas, self.eps, self.step_size, self.gamma = lr, betas, eps, step_size, gamma
        self.exp_avg = torch.zeros_like(model._flat)
        self.exp_avg_sq = torch.zeros_like(model._flat)
        self.state = torch.zeros(4, dtype=torch.float32, device=model._flat.device)
        self.process_group = process_group
        if max_grad_norm is not None and math.isnan(float(max_grad_norm)):
            raise ValueError('max_grad_norm is NaN')
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self.guard = self._scratch = self._norm_table = None
        if self.guarded:
            self._alloc_guard()
        # consecutive StyleTransferModel.train_iteration calls may now overlap on two lanes (two gradient buffers): this
        # optimizer joins them in step()
        model.concurrent_accumulation = True

    @property
    def guarded(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _alloc_guard(self):
        """The guard record and the partial sums of the norm: allocated once, never in step()."""
        flat = self.model._flat
        if self.guard is None or self.guard.device != flat.device:
            self.guard = torch.zeros(8, dtype=torch.float32, device=flat.device)
        nbytes = _native.get().lib.mst_grad_guard_scratch_bytes(flat.numel())
        if self._scratch is None or self._scratch.device != flat.device or self._scratch.numel() * 8 < nbytes:
            self._scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=flat.device)

    def all_reduce_grads(self):
        if self.process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                              and torch.distributed.get_world_size() > 1):
            torch.distributed.all_reduce(self.model._gflat, op=torch.distributed.ReduceOp.SUM, group=self.process_group)

    def step(self, zero_grad=True):
        m = self.model
        m._sync_flat()
        g2 = m.join_lanes() if hasattr(m, 'join_lanes') else None
        if g2 is not None and (self.process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                                                  and torch.distributed.get_world_size() > 1)):
            m._gflat.add_(g2); g2.zero_(); g2 = None          # one buffer for the collective
        self.all_reduce_grads()
        n = m._flat.numel()
        P = _native.ptr
        if self.guarded:
            # after the fold and the all-reduce above: the guard sees the summed gradient of all ranks, every rank decides alike
            if self.guard is None or self.guard.device != m._flat.device or self._scratch.numel() * 4096 < n:
                self._alloc_guard()
            _native.check(_native.get().lib.mst_adam_step_guarded(
                P(m._flat), P(m._gflat), P(g2), P(self.exp_avg), P(self.exp_avg_sq), n, P(self.state), P(self.guard),
                self._scratch.data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps, self.step_size, self.gamma,
                0. if self.max_grad_norm is None else float(self.max_grad_norm), int(self.skip_nonfinite), int(zero_grad),
                _native.current_stream(m._flat.device)), 'mst_adam_step_guarded')
            if g2 is not None and not zero_grad:
                m._gflat.add_(g2); g2.zero_()                 # keep the accumulated sum visible in p.grad
            return
        if g2 is not None:
            _native.check(_native.get().lib.mst_adam_step2(P(m._flat), P(m._gflat), P(g2), P(self.exp_avg), P(self.exp_avg_sq), n,
                                                           P(self.state), self.lr, self.betas[0], self.betas[1], self.eps,
                                                           self.step_size, self.gamma, int(zero_grad),
                                                           _native.current_stream(m._flat.device)), 'mst_adam_step2')
            if not zero_grad:
                m._gflat.add_(g2); g2.zero_()                 # keep the accumulated sum visible in p.grad
            return
        _native.check(_native.get().lib.mst_adam_step(P(m._flat), P(m._gflat), P(self.exp_avg), P(self.exp_avg_sq), n,
                                                      P(self.state), self.lr, self.betas[0], self.betas[1], self.eps,
                                                      self.step_size, self.gamma, int(zero_grad),
                                                      _native.current_stream(m._flat.device)), 'mst_adam_step')

    def zero_grad(self):
        g2 = self.model.join_lanes() if hasattr(self.model, 'join_lanes') else None
        if g2 is not None:
            g2.zero_()
        self.model._gflat.zero_()

    # ---- guard read-outs (they synchronise: meant for flush time, not for every step)
    def guard_stats(self):
        """The guard record as a dict: `norm` / `coef` / `skipped` of the last step, `steps_skipped`, `steps_clipped`, and the
        largest finite norm so far (`largest_norm`).  None when the guard is off.  Synchronises."""
        if self.guard is None:
            return None
        w = self.guard.cpu().tolist()
        d = dict(zip(self.GUARD_KEYS, w))
        d['skipped'] = bool(d['skipped'])
        d['steps_skipped'], d['steps_clipped'] = int(d['steps_skipped']), int(d['steps_clipped'])
        return d

    def grad_norms(self):
        """{state_dict name: L2 norm of that tensor's accumulated gradient} (mst_grad_norms, one launch, lane 1's share
        included).  The lanes are waited for, not consumed: a step() afterwards still sees both.  Synchronises."""
        m = self.model
        m._sync_flat()
        dev = m._flat.device
        if self._norm_table is None or self._norm_table[0].device != dev:
            names, offs, lens = [], [], []
            for (name, p), off in zip(m.named_parameters(), m._offsets):
                names.append(name); offs.append(off); lens.append(p.numel())
            self._norm_table = (torch.tensor([offs, lens], dtype=torch.int64).to(dev), names,          # uploaded once
                                torch.zeros(len(names), dtype=torch.float32, device=dev))
        table, names, out = self._norm_table
        if hasattr(m, 'join_lanes_keep'):
            m.join_lanes_keep()
        lanes = m.__dict__.get('_lane_list')
        g2 = lanes[1]['grad'] if lanes and lanes[1]['dirty'] else None
        _native.check(_native.get().lib.mst_grad_norms(_native.ptr(m._gflat), _native.ptr(g2), table[0].data_ptr(),
                                                       table[1].data_ptr(), len(names), _native.ptr(out),
                                                       _native.current_stream(dev)), 'mst_grad_norms')
        return dict(zip(names, out.cpu().tolist()))

    # ---- snapshots: a whole-module snapshot carries the model, not the moments or the StepLR step count
    HYPER = ('lr', 'betas', 'eps', 'step_size', 'gamma', 'max_grad_norm', 'skip_nonfinite')

    def state_dict(self):
        guard = self.guard if self.guard is not None else torch.zeros(8, dtype=torch.float32)
        return dict(exp_avg=self.exp_avg.detach().cpu().clone(), exp_avg_sq=self.exp_avg_sq.detach().cpu().clone(),
                    state=self.state.detach().cpu().clone(), guard=guard.detach().cpu().clone(),
                    hyper={k: getattr(self, k) for k in self.HYPER})

    def load_state_dict(self, sd):
        self.model._sync_flat()
        n = self.model._flat.numel()
        for k in ('exp_avg', 'exp_avg_sq'):
            if sd[k].numel() != n:
                raise ValueError(f'optimizer state {k} has {sd[k].numel()} elements, the model has {n} parameters')
        if sd['state'].numel() != self.state.numel() or sd['guard'].numel() != 8:
            raise ValueError('optimizer state: `state` / `guard` have the wrong size')
        for k, v in sd['hyper'].items():
            if k not in self.HYPER:
                raise ValueError(f'unknown hyper-parameter {k!r}')
            setattr(self, k, tuple(v) if k == 'betas' else v)
        self.exp_avg.copy_(sd['exp_avg'].reshape(-1))
        self.exp_avg_sq.copy_(sd['exp_avg_sq'].reshape(-1))
        self.state.copy_(sd['state'].reshape(-1))
        if self.guarded:
            self._alloc_guard()
            self.guard.copy_(sd['guard'].reshape(-1))
