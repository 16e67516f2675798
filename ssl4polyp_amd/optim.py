"""Fused AdamW + gradient statistics over the engine's flat parameter storage.

Same update rule and hyper-parameter surface as ``torch.optim.AdamW`` as the reference uses it
(train_classification.py:5766-5768: two groups head/backbone, default betas; mae/main_pretrain.py:217-218:
decay / no-decay groups from timm ``add_weight_decay``, betas (0.9, 0.95)), but one HIP launch per
contiguous flat segment instead of ~150 tensors, and the same launch refreshes the bf16 shadow weights the
MFMA GEMMs read.  ``grad_stats`` replaces the per-parameter host-synchronising loops of
train_classification.py:1437-1454 (_compute_grad_norm) and mae/util/misc.py:387-400 (detect_grad_anomalies)
with one pass that stays on the device.  ``step(max_norm=...)`` clips by global norm where the reference calls
``clip_grad_norm_`` between ``unscale_`` and ``step`` (mae/util/misc.py:268-279), and ``grad_norms`` returns the
per-group norms of train_classification.py:4534-4544: one deterministic f64 pass, the coefficient folded into the factor
the update already multiplies every gradient by.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import contextlib
import ctypes

import torch

from . import _lib
from .cohorts import CohortPlan
from .engine import _ptr, _stream


def add_weight_decay(model, weight_decay=1e-5, skip_list=()):
    """timm 0.4.12 optim_factory.add_weight_decay (main_pretrain.py:217): 1-D params and biases get no decay."""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if len(param.shape) == 1 or name.endswith(".bias") or name in skip_list:
            no_decay.append(param)
        else:
            decay.append(param)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, model, params=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 overlap_forward: bool = False, per_parameter_steps: bool = False):
        """`model`: an ssl4polyp_amd module (owns the flat storage).  `params`: iterable of parameters or of
        torch-style param-group dicts (default: all parameters of the model).
        per_parameter_steps: by default (False) the parameters of a param group SHARE ONE STEP: every step() advances every
        group's bias corrections, whether its parameters had a gradient or not.  That equals torch.optim.AdamW as long as the set of
        parameters with a gradient never changes, which holds for one --finetune_mode per run.  True: torch's rule -- a parameter's
        step counts the optimizer steps in which it had a gradient and that the loss scaler did not skip; a parameter that is
        unfrozen mid-run starts its bias corrections at 1, one that is frozen and unfrozen again continues, one that was never
        updated has no state.  A group then owns one device record per cohort of parameters with a common history (cohorts.py); the
        update kernels are the same, and with a constant gradient pattern so are the bits.  The plan is fixed while a GraphedStep
        lives: take one eager step in a new stage, then capture again.
        overlap_forward: run the update on the engine's side stream, block by block in forward order, and let the next
        forward wait per block (the update is HBM-bound, the forward GEMMs MFMA-bound: ~0.5 ms of the step hides).
        The model's forward / state_dict and this optimizer's state_dict / grad_stats wait for the update by
        themselves; code that reads parameter tensors directly right after step() must call `sync()` first."""
        self._rt = model._rt
        self.overlap_forward = bool(overlap_forward)
        self.per_parameter_steps = bool(per_parameter_steps)
        self._cohorts: Optional[CohortPlan] = None
        if params is None:
            params = list(model.parameters())
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._M: Dict[str, torch.Tensor] = {}
        self._V: Dict[str, torch.Tensor] = {}
        self._plan = None
        self._plan_key = None
        self.grad_scale = 1.0  # e.g. 1/world_size when gradients were all-reduced with SUM
        self.grad_sync = None  # parallel.GradSync: waited on before the update

    # -- planning: contiguous flat segments per group --------------------------------------------
    def _ensure_state(self):
        f = self._rt.flat
        if f is None or not f.P:
            raise _lib.PolypMaeError("FusedAdamW: run a forward pass (or model._rt.ensure(device)) before step()")
        key = (id(f.P["mat"]), id(f.P["vec"]))
        if self._plan_key != key:
            old_M, old_V = self._M, self._V
            self._M = {r: torch.zeros_like(t) for r, t in f.P.items()}
            self._V = {r: torch.zeros_like(t) for r, t in f.P.items()}
            for r in old_M:  # re-materialised storage: carry the moments over
                if old_M[r].numel() == self._M[r].numel():
                    self._M[r].copy_(old_M[r])
                    self._V[r].copy_(old_V[r])
            self._plan_key = key
            self._plan = None
        return f

    def _segments(self, f, group):
        """[(region, lo, hi)] covering the group's parameters that currently have a gradient."""
        return self._segments_of(f, group["params"])

    def _segments_of(self, f, params):
        idx = {id(p): i for i, p in enumerate(f.params)}
        items = []
        for p in params:
            if p.grad is None:
                continue
            i = idx.get(id(p))
            if i is None:
                raise _lib.PolypMaeError("FusedAdamW: parameter does not belong to the model's flat storage")
            if not f.grad_is_flat(f.names[i]):  # foreign gradient tensor: stage it into the flat range
                f.grad_view(f.names[i]).copy_(p.grad)
            A = f.ALIGN
            items.append((f.region[i], f.offset[i], f.offset[i] + (f.numel[i] + A - 1) // A * A))
        items.sort()
        segs = []
        for r, lo, hi in items:
            if segs and segs[-1][0] == r and segs[-1][2] == lo:
                segs[-1] = (r, segs[-1][1], hi)
            else:
                segs.append((r, lo, hi))
        return segs

    # -- device-resident hyper-parameters (so that a captured step can be replayed as a hipGraph) ---------------
    HYPER_STRIDE = 16  # floats per group: lr, beta1, beta2, eps, wd, grad_scale, step, bc1, rsqrt_bc2 (pm_adamw_dev)

    def _host_hyper(self):
        rows = []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            rows.append((float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                         float(self.grad_scale)))
        if self.per_parameter_steps:  # one row per record: the group's values into each of its cohorts' records
            return [rows[g] for g in self._plan_cohorts().group_of]
        return rows

    def _n_records(self) -> int:
        return self._plan_cohorts().n_records if self.per_parameter_steps else len(self.param_groups)

    def sync_hyper(self, force: bool = False):
        """Push lr / betas / eps / weight_decay / grad_scale to the device records when they changed on the host.
        Called automatically by step() outside stream capture; call it yourself between graph replays."""
        f = self._ensure_state()
        rows = self._host_hyper()
        if getattr(self, "_hyper", None) is None or self._hyper.device != f.device:
            moved = getattr(self, "_hyper", None)  # the records on the device the storage left, if any
            self._hyper = torch.zeros(len(rows), self.HYPER_STRIDE, dtype=torch.float32, device=f.device)
            if self.per_parameter_steps and moved is not None and moved.shape[0] == len(rows):
                # the device records are authoritative (steps the loss scaler skipped are not in the host mirrors): carry them over
                self._hyper[:, 6:11] = moved[:, 6:11].to(f.device)
            elif self.per_parameter_steps:  # (first step, or after load_state_dict: the plan's steps are the loaded ones)
                self._hyper[:, 6] = torch.tensor(self._plan_cohorts().steps, dtype=torch.float32)
            else:
                for gi, group in enumerate(self.param_groups):  # resume: restore the step counter
                    self._hyper[gi, 6] = float(group.get("step", 0))
            self._hyper_host = None
        if force or rows != self._hyper_host:
            # The MAE loop changes lr EVERY iteration (engine_pretrain.py:47-48): the upload must not block the host, or
            # each step would wait for the whole backward to drain before AdamW and the next forward can be enqueued.
            # Pinned staging slots, asynchronous copy on the current stream, one event per slot (a slot is rewritten
            # only after its previous copy has executed: four steps of run-ahead before the host could ever wait here).
            if f.device.type == "cuda":
                if getattr(self, "_hyper_pin", None) is None or self._hyper_pin[0].shape[0] != len(rows):
                    self._hyper_pin = [torch.empty(len(rows), 6, dtype=torch.float32).pin_memory() for _ in range(4)]
                    self._hyper_pin_ev = [None] * 4
                    self._hyper_slot = 0
                i = self._hyper_slot
                self._hyper_slot = (i + 1) % 4
                if self._hyper_pin_ev[i] is not None:
                    self._hyper_pin_ev[i].synchronize()
                self._hyper_pin[i].copy_(torch.tensor(rows, dtype=torch.float32))
                self._hyper[:, :6].copy_(self._hyper_pin[i], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(f.device))
                self._hyper_pin_ev[i] = ev
            else:
                self._hyper[:, :6].copy_(torch.tensor(rows, dtype=torch.float32))
            self._hyper_host = rows

    # -- clipping by global norm and per-group norms (pm_grad_norms / pm_grad_clip) -------------------------------
    def _clip_buffers(self, f, n_segs):
        """Workspace, f64 sums, f32 triple and f64 record of the norm kernels: allocated once (outside capture: a GraphedStep runs
        its eager warm-up steps first), at fixed addresses, so that a captured step replays them."""
        G, R = len(self.param_groups), self._n_records()  # (R == G unless per_parameter_steps: one sum per record)
        size = _lib.workspace_bytes("pm_grad_norms_workspace", n_segs, R)
        b = getattr(self, "_clip_buf", None)
        if b is None or b["ws"].device != f.device or b["ws"].numel() * 8 < size or b["sumsq"].numel() != R:
            b = self._clip_buf = {"ws": torch.zeros((size + 7) // 8, dtype=torch.float64, device=f.device),
                                  "sumsq": torch.zeros(R, dtype=torch.float64, device=f.device),
                                  "stats": torch.zeros(3, dtype=torch.float32, device=f.device),
                                  "record": torch.zeros(G + 3, dtype=torch.float64, device=f.device),
                                  "norms": torch.zeros(G + 3, dtype=torch.float64, device=f.device)}
        return b

    def _grad_segment_array(self, f, stat_segs):
        """pm_grad_segment array of [(group, region, lo, hi)], rebuilt only when the segments or the gradient buffers change."""
        key = (tuple(stat_segs),) + tuple(f.G[r].data_ptr() for r in ("mat", "vec"))
        if getattr(self, "_gseg_key", None) != key:
            arr = (_lib.GradSegment * len(stat_segs))()
            for i, (gi, r, lo, hi) in enumerate(stat_segs):
                arr[i] = _lib.GradSegment(_ptr(f.G[r][lo:hi]), hi - lo, gi)
            self._gseg_key, self._gseg_args = key, arr
        return self._gseg_args

    def _grad_norms_pass(self, f, stat_segs, stats=None):
        """The statistics pass on the current stream: per-group f64 sums into the optimizer's buffer, the f32 triple into `stats`
        (default: the optimizer's own).  Returns the buffers."""
        b = self._clip_buffers(f, len(stat_segs))
        _lib.check(self._rt.k.lib.pm_grad_norms(self._grad_segment_array(f, stat_segs), len(stat_segs), self._n_records(),
                                                _ptr(b["ws"]), b["ws"].numel() * 8, _ptr(b["sumsq"]),
                                                _ptr(stats if stats is not None else b["stats"]), _stream()), "pm_grad_norms")
        return b

    @property
    def last_clip(self) -> Optional[torch.Tensor]:
        """Device record of the last step taken with `max_norm`, f64 [G + 3]: the norm of each group's gradient as the update
        consumed it (times grad_scale, divided by the loss scale), the total norm before clipping, the clip coefficient,
        max_norm.  None before the first clipped step.  The tensor is rewritten by every clipped step: clone it to keep a value."""
        b = getattr(self, "_clip_buf", None)
        if b is None or not getattr(self, "_clip_seen", False):
            return None
        if getattr(self, "_clip_ev", None) is not None:  # written by an overlapped step, on the side stream
            torch.cuda.current_stream(b["record"].device).wait_event(self._clip_ev)
        return b["record"]

    @torch.no_grad()
    def grad_norms(self, loss_scaler: "Optional[LossScaler]" = None) -> torch.Tensor:
        """f64 device tensor [G + 1]: the gradient norm of every param group, then the global norm (no host sync) -- of the
        gradient as the update will consume it: times grad_scale (so on N ranks it is the norm of the averaged gradient), and
        divided by `loss_scaler`'s current scale when one is given.  What the reference's `_compute_grad_norm(group["params"])`
        returns after scaler.unscale_ (train_classification.py:4534-4544).  A group without gradients reports 0."""
        f = self._ensure_state()
        self._rt.wait_updates()
        if self.grad_sync is not None:
            self.grad_sync.wait()
        G = len(self.param_groups)
        capturing = f.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if not capturing or getattr(self, "_hyper", None) is None:
            self.sync_hyper()
        stat_segs = [(gi, r, lo, hi) for gi, group in enumerate(self.param_groups) for r, lo, hi in self._segments(f, group)]
        if not stat_segs:
            return torch.zeros(G + 1, dtype=torch.float64, device=f.device)
        # (per_parameter_steps: the segments are tagged by their group's FIRST record, g -- a parameter that has its first gradient
        # has no cohort before the step -- and summed per group like any other tagging)
        b = self._grad_norms_pass(f, stat_segs)
        self._clip_call(b, 0.0, 0, 0, b["norms"])
        out = b["norms"][:G + 1].clone()
        if loss_scaler is not None and loss_scaler.enabled:
            state, _ = loss_scaler._device_state(f.device)
            out /= state[0].double()
        return out

    @torch.no_grad()
    def step(self, closure=None, loss_scaler: "Optional[LossScaler]" = None, max_norm: Optional[float] = None):
        """loss_scaler: the gradients carry its loss scale (precision mode fp16).  The update then starts with one statistics
        pass over them and `pm_loss_scale_update` -- found_inf, the skip flag and 1/scale go into the device-side hyper records,
        the scale moves (GradScaler.step + update, train_classification.py:4545-4546) -- and `pm_adamw_dev` unscales inside
        the update or returns untouched on a non-finite step: no host read-back anywhere.
        max_norm: clip the gradients by global norm first, `torch.nn.utils.clip_grad_norm_(params, max_norm)` between unscale_ and
        step (mae/util/misc.py:268-279), on the device: one deterministic statistics pass (`pm_grad_norms`; under a loss scaler
        it replaces the `pm_grad_stats` pass, the gradients are read once), `pm_loss_scale_update`, `pm_grad_clip` -- which folds
        min(1, max_norm / (norm + 1e-6)) into the factor the unchanged update kernels multiply every gradient by -- then the
        update as without it.  The norm is that of the gradient the update consumes (times grad_scale, divided by the loss
        scale); `last_clip` holds the per-group norms, the total, the coefficient.  The flat gradients themselves are not
        rewritten.  A non-finite norm without a loss scaler gives NaN parameters, as clip_grad_norm_ + step does.  max_norm is a
        kernel argument: a GraphedStep replays the value it was captured with."""
        loss = None
        if max_norm is not None and not float(max_norm) > 0.0:
            raise _lib.PolypMaeError(f"FusedAdamW.step: max_norm must be positive, got {max_norm}")
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        f = self._ensure_state()
        rt = self._rt
        rt.wait_updates()  # a previous overlapped update (reads the hyper records and the gradients)
        if self.grad_sync is not None:
            self.grad_sync.wait()
        capturing = f.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if not capturing or getattr(self, "_hyper", None) is None:
            self.sync_hyper()
        lib = self._rt.k.lib
        overlap = self.overlap_forward and not capturing and f.device.type == "cuda"
        work = []  # (group index, region, lo, hi); per_parameter_steps: (record index, ...), see _cohort_work
        if self.per_parameter_steps:
            work = self._cohort_work(f, capturing)
        else:
            for gi, group in enumerate(self.param_groups):
                group["step"] = int(group.get("step", 0)) + 1  # host mirror (the device record is authoritative)
                for r, lo, hi in self._segments(f, group):
                    work.append((gi, r, lo, hi))
        n_rec = self._n_records()
        scaled = loss_scaler is not None and loss_scaler.enabled
        clip = max_norm is not None and bool(work)
        stat_segs = list(work) if (scaled or clip) else []
        if not scaled and (getattr(self, "_scaler_used", False) or (getattr(self, "_clip_used", False) and not clip)):
            # a scaler or max_norm was dropped: clear the skip flag / the factor it left in [10]
            self._hyper[:, 9:11] = 0.0
            self._scaler_used = False
        self._clip_used = clip
        if overlap:
            # forward order: vectors first, then the matrices by offset, cut at the block boundaries so that the next
            # forward can start on block 0 while the later blocks are still being updated
            cuts = sorted(f.offset[i] for i, n in enumerate(f.names) if n.endswith("attn.qkv.weight"))
            split = []
            for gi, r, lo, hi in work:
                if r != "mat":
                    split.append((gi, r, lo, hi))
                    continue
                pts = [lo] + [c for c in cuts if lo < c < hi] + [hi]
                split += [(gi, r, a, b) for a, b in zip(pts[:-1], pts[1:])]
            work = sorted(split, key=lambda w: (w[1] != "vec", w[2]))
            main = torch.cuda.current_stream(f.device)
            side = rt.k.side_stream(f.device)
            ev = self._event(-1, side)
            ev.record(main)
            if scaled or clip or not work:
                side.wait_event(ev)
            stream_ctx = torch.cuda.stream(side)
        else:
            stream_ctx = contextlib.nullcontext()
        with stream_ctx:
            if scaled:
                state, stats = loss_scaler._device_state(f.device)
                if clip:  # one pass gives the per-group sums AND the triple the scale update reads
                    self._grad_norms_pass(f, stat_segs, stats)
                else:
                    stats.zero_()
                    for _, r, lo, hi in stat_segs:
                        _lib.check(lib.pm_grad_stats(_ptr(f.G[r][lo:hi]), hi - lo, _ptr(stats), _stream()), "pm_grad_stats")
                _lib.check(lib.pm_loss_scale_update(_ptr(state), _ptr(stats), _ptr(self._hyper), n_rec,
                                                    loss_scaler.growth_factor, loss_scaler.backoff_factor,
                                                    loss_scaler.growth_interval, _stream()), "pm_loss_scale_update")
                self._scaler_used = True
            elif clip:
                self._grad_norms_pass(f, stat_segs)
            if clip:
                b = self._clip_buf
                self._clip_call(b, float(max_norm), 1, 1 if scaled else 0, b["record"])
                self._clip_seen = True
                self._clip_ev = None
                if overlap:  # the record is written on the side stream: `last_clip` makes its reader's stream wait for it
                    self._clip_ev = self._event(-2, side)
                    self._clip_ev.record(side)
            if overlap and work:
                # the whole update in ONE C call: [wait for the main stream's event,] tick, then launch + done event per segment
                segs, events = self._segment_array(f, work, side)
                wait = None if (scaled or clip) else ev.cuda_event
                if self.per_parameter_steps:
                    tick_dev, tick_host = self._tick
                    _lib.check(lib.pm_adamw_segments_list(segs, len(work), _ptr(self._hyper), n_rec, _ptr(tick_dev), tick_host,
                                                          len(tick_host), wait, _stream(), self.OVERLAP_MAX_BLOCKS),
                               "pm_adamw_segments_list")
                else:
                    _lib.check(lib.pm_adamw_segments(segs, len(work), _ptr(self._hyper), len(self.param_groups), wait, _stream(),
                                                     self.OVERLAP_MAX_BLOCKS), "pm_adamw_segments")
                rt.pending_updates += [(r, lo, hi, done) for (_, r, lo, hi), done in zip(work, events)]
                return loss
            if self.per_parameter_steps:
                if not work:  # nothing has a gradient: no record advances
                    return loss
                tick_dev, tick_host = self._tick
                _lib.check(lib.pm_adamw_tick_list(_ptr(self._hyper), n_rec, _ptr(tick_dev), tick_host, len(tick_host), _stream()),
                           "pm_adamw_tick_list")
            else:
                _lib.check(lib.pm_adamw_tick(_ptr(self._hyper), len(self.param_groups), _stream()), "pm_adamw_tick")
            for gi, r, lo, hi in work:
                shadow = f.S[lo:hi] if (r == "mat" and f.S is not None) else None
                _lib.check(lib.pm_adamw_dev(_ptr(f.P[r][lo:hi]), _ptr(f.G[r][lo:hi]), _ptr(self._M[r][lo:hi]),
                                            _ptr(self._V[r][lo:hi]), _ptr(shadow),
                                            _lib.dtype_code(shadow.dtype) if shadow is not None else 0, hi - lo,
                                            _ptr(self._hyper[gi]), _stream()), "pm_adamw_dev")
        return loss

    # -- per_parameter_steps: cohorts of parameters with a common step history (cohorts.py) ---------------------------------------
    def _plan_cohorts(self) -> CohortPlan:
        if self._cohorts is None:
            self._cohorts = CohortPlan(len(self.param_groups))
        return self._cohorts

    def _cohort_keys(self, f):
        """Per param group, the flat-storage index of every parameter (the plan's keys), and {key: parameter}."""
        idx = {id(p): i for i, p in enumerate(f.params)}
        groups, by_key = [], {}
        for group in self.param_groups:
            keys = []
            for p in group["params"]:
                i = idx.get(id(p))
                if i is None:
                    raise _lib.PolypMaeError("FusedAdamW: parameter does not belong to the model's flat storage")
                keys.append(i)
                by_key[i] = p
            groups.append(keys)
        return groups, by_key

    def _cohort_work(self, f, capturing):
        """Advance the plan by this step's `p.grad is None` pattern and return the work list [(record, region, lo, hi)].  New and
        split records are created here (device copies of the rows they start from), the group's hyper-parameters go into them, and
        the device lists the kernels read (`_tick`: the records to advance; `_group_of`: record -> group) follow.  Under capture
        nothing of that may change: the plan is fixed while a graph lives."""
        plan = self._plan_cohorts()
        groups, by_key = self._cohort_keys(f)
        active = {k for k, p in by_key.items() if p.grad is not None}
        if capturing:
            if getattr(self, "_hyper", None) is None or plan.preview(groups, active):
                raise _lib.PolypMaeError("FusedAdamW(per_parameter_steps=True): the set of parameters with a gradient changed; the "
                                         "cohort plan is fixed while a graph lives -- take one eager step in the new stage, then "
                                         "capture again")
        copies, tick = plan.advance(groups, active)
        R = plan.n_records
        if self._hyper.shape[0] != R:  # (never under capture: preview() refused above)
            grown = torch.zeros(R, self.HYPER_STRIDE, dtype=torch.float32, device=self._hyper.device)
            grown[:self._hyper.shape[0]] = self._hyper
            for dst, src in copies:  # a split: the idle part's record starts as a copy (step, bias corrections, flags)
                grown[dst] = grown[src]
            self._hyper = grown
            self._hyper_host = None
        if not capturing:
            self.sync_hyper()
        self._set_device_lists(plan, tick, capturing)
        work = []
        for by_record in plan.records_of(groups, active):
            for rec in sorted(by_record):
                work += [(rec, r, lo, hi) for r, lo, hi in self._segments_of(f, [by_key[k] for k in by_record[rec]])]
        return work

    def _set_device_lists(self, plan, tick, capturing):
        dev = self._hyper.device
        key = tuple(plan.group_of)
        if getattr(self, "_group_of_key", None) != (key, dev):
            host = (ctypes.c_int * len(key))(*key)
            self._group_of = (torch.tensor(key, dtype=torch.int32).to(dev), host)
            self._group_of_key = (key, dev)
        tick = tuple(tick)
        if getattr(self, "_tick_key", None) != (tick, dev, len(key)):
            if capturing:
                raise _lib.PolypMaeError("FusedAdamW(per_parameter_steps=True): the records to advance changed under capture")
            old = getattr(self, "_tick", None)
            buf = old[0] if old is not None and old[0].device == dev and old[0].numel() >= max(len(key), 1) else \
                torch.zeros(max(len(key), 16), dtype=torch.int32, device=dev)  # fixed address while the record count stands
            if tick:
                buf[:len(tick)].copy_(torch.tensor(tick, dtype=torch.int32))
            self._tick = (buf, (ctypes.c_int * len(tick))(*tick))
            self._tick_key = (tick, dev, len(key))

    def _clip_call(self, b, max_norm, clip, scaled, record):
        """pm_grad_clip, or its sibling over cohort records (sums per record -> per group, the coefficient into every record)."""
        lib = self._rt.k.lib
        G = len(self.param_groups)
        if self.per_parameter_steps:
            plan = self._plan_cohorts()
            if getattr(self, "_group_of_key", None) != (tuple(plan.group_of), self._hyper.device):
                self._set_device_lists(plan, (getattr(self, "_tick_key", None) or ((),))[0], False)
            group_dev, group_host = self._group_of
            _lib.check(lib.pm_grad_clip_cohorts(_ptr(b["sumsq"]), _ptr(self._hyper), plan.n_records, _ptr(group_dev), group_host, G,
                                                max_norm, clip, scaled, _ptr(record), _stream()), "pm_grad_clip_cohorts")
        else:
            _lib.check(lib.pm_grad_clip(_ptr(b["sumsq"]), _ptr(self._hyper), G, max_norm, clip, scaled, _ptr(record), _stream()),
                       "pm_grad_clip")

    # -- the overlapped update's launcher arguments (pm_adamw_segments) -----------------------------------------
    # Workgroups per launch of the overlapped update (pm_adamw_grid; 0 = the full grid, which the inline path keeps).  Chosen by
    # step rate from 64 / 128 / 256 / 512 / 1024 / unbounded on the cls headline and on MAE, the parent alternating in the same
    # job (docs/EXPERIMENT_LOG.md, "AdamW footprint"): 256 is the smallest grid that still runs the update at HBM rate alone
    # (64 and 128 fall below it and lose 4 % / 2 % of the step), and the best or equal-best on both workloads.
    OVERLAP_MAX_BLOCKS = 256

    def _event(self, i, side):
        """Event number i of the overlapped path, created once (-1: the main stream's fork event; i >= 0: segment i's done event).
        step() waits for every pending update before it records any of them again."""
        cache = self.__dict__.setdefault("_events", {})
        e = cache.get(i)
        if e is None:
            e = cache[i] = torch.cuda.Event()
            e.record(side)  # (materialises the hipEvent_t handle)
        return e

    def _segment_array(self, f, work, side):
        """(pm_adamw_segment array, done events) of `work`, rebuilt only when the segments or the buffers behind them change."""
        S = f.S
        key = (tuple(work), S.dtype if S is not None else None, self._hyper.data_ptr(), _ptr(S)) + \
            tuple(t[r].data_ptr() for r in ("mat", "vec") for t in (f.P, f.G, self._M, self._V))
        if getattr(self, "_seg_key", None) != key:
            events = [self._event(i, side) for i in range(len(work))]
            segs = (_lib.AdamwSegment * len(work))()
            for i, (gi, r, lo, hi) in enumerate(work):
                shadow = S[lo:hi] if (r == "mat" and S is not None) else None
                segs[i] = _lib.AdamwSegment(_ptr(f.P[r][lo:hi]), _ptr(f.G[r][lo:hi]), _ptr(self._M[r][lo:hi]), _ptr(self._V[r][lo:hi]),
                                            _ptr(shadow), _lib.dtype_code(shadow.dtype) if shadow is not None else 0, hi - lo,
                                            _ptr(self._hyper[gi]), events[i].cuda_event)
            self._seg_key, self._seg_args = key, (segs, events)
        return self._seg_args

    def sync(self) -> None:
        """Make the current stream wait for an overlapped update (no-op otherwise)."""
        self._rt.wait_updates()

    def grad_stats(self) -> torch.Tensor:
        """Device tensor [sum(g^2), #NaN, #Inf] over every gradient of every group (no host sync)."""
        f = self._ensure_state()
        self._rt.wait_updates()
        out = torch.zeros(3, dtype=torch.float32, device=f.device)
        lib = self._rt.k.lib
        for group in self.param_groups:
            for r, lo, hi in self._segments(f, group):
                _lib.check(lib.pm_grad_stats(_ptr(f.G[r][lo:hi]), hi - lo, _ptr(out), _stream()), "pm_grad_stats")
        return out

    # -- torch.optim.AdamW-compatible (de)serialisation --------------------------------------------
    def state_dict(self, host: bool = False):
        """torch.optim.AdamW's layout.  host=True: the moments are copied to host memory HERE, on the calling thread's current
        stream (two D2H copies of the flat ranges, then per-parameter views) -- what a checkpoint writer thread needs: nothing
        device-side outlives the call and no device clone of the 2 x f32 moments is made."""
        self._rt.wait_updates()
        f = self._rt.flat
        idx = {id(p): i for i, p in enumerate(f.params)} if f is not None else {}
        state, groups, k = {}, [], 0
        M, V = self._M, self._V
        if host and M:
            M = {r: t.detach().cpu() for r, t in M.items()}
            V = {r: t.detach().cpu() for r, t in V.items()}
        psteps = None
        if self.per_parameter_steps:
            # torch's layout exactly: an entry per UPDATED parameter, its step the cohort's, read from the device records (one
            # D2H read: steps the loss scaler skipped are not in it); no entry for a parameter that was never updated
            records = self._hyper[:, 6].tolist() if getattr(self, "_hyper", None) is not None else None
            psteps = self._plan_cohorts().parameter_steps(records)
        for group in self.param_groups:
            ids = []
            for p in group["params"]:
                i = idx.get(id(p))
                if i is not None and M and (psteps is None or i in psteps):
                    r, lo, n = f.region[i], f.offset[i], f.numel[i]
                    state[k] = {"step": torch.tensor(float(group.get("step", 0) if psteps is None else psteps[i])),
                                "exp_avg": M[r][lo:lo + n].view(p.shape).clone(),
                                "exp_avg_sq": V[r][lo:lo + n].view(p.shape).clone()}
                ids.append(k)
                k += 1
            g = {kk: v for kk, v in group.items() if kk != "params"}
            g["params"] = ids
            groups.append(g)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        f = self._ensure_state()
        self._rt.wait_updates()
        idx = {id(p): i for i, p in enumerate(f.params)}
        psteps = {}  # per_parameter_steps: flat index -> the parameter's own step
        for group, saved in zip(self.param_groups, sd["param_groups"]):
            for kk, v in saved.items():
                if kk != "params" and not (self.per_parameter_steps and kk == "step"):
                    group[kk] = v
            for p, k in zip(group["params"], saved["params"]):
                st = sd["state"].get(k)
                if st is None:
                    continue
                i = idx[id(p)]
                r, lo, n = f.region[i], f.offset[i], f.numel[i]
                self._M[r][lo:lo + n].copy_(st["exp_avg"].reshape(-1))
                self._V[r][lo:lo + n].copy_(st["exp_avg_sq"].reshape(-1))
                if self.per_parameter_steps:
                    psteps[i] = float(st["step"])
                else:
                    group["step"] = int(float(st["step"]))
        if self.per_parameter_steps:  # the cohorts are rebuilt from the per-parameter steps (torch.optim.AdamW's dict loads as well)
            self._cohorts = CohortPlan.from_steps(self._cohort_keys(f)[0], psteps)
            self._group_of_key = self._tick_key = None
        self._hyper = None  # rebuild the device records (incl. the step counters) at the next step()


class _ScaleLossFn(torch.autograd.Function):
    """loss * scale and d loss * scale, the scale read from DEVICE memory by the kernel (pm_scale): no host value is baked in."""

    @staticmethod
    def forward(ctx, loss, scale):
        lib = _lib.load()
        x = loss.reshape(1).contiguous().float()
        out = torch.empty_like(x)
        _lib.check(lib.pm_scale(_ptr(x), _ptr(scale), _ptr(out), 1, _stream()), "pm_scale")
        ctx.scale = scale
        return out.reshape(())

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        d = dout.reshape(1).contiguous().float()
        out = torch.empty_like(d)
        _lib.check(lib.pm_scale(_ptr(d), _ptr(ctx.scale), _ptr(out), 1, _stream()), "pm_scale")
        return out.reshape(()), None


class LossScaler:
    """Dynamic loss scaling for precision mode "fp16", resident on the device.

    Same surface and arithmetic as the ``torch.cuda.amp.GradScaler`` of the reference's AMP loops
    (train_classification.py:4533-4546: ``scaler.scale(loss).backward(); scaler.unscale_(opt); scaler.step(opt); scaler.update()``;
    engine_pretrain.py:65-72 through mae/util/misc.py:252-282), same defaults (65536, x2 after 2000 clean steps, x0.5 after a
    non-finite one).  Different mechanics: GradScaler.step reads ``found_inf`` back to the host before it decides whether to call
    ``optimizer.step()`` -- one pipeline drain per step; here the decision, the unscaling and the scale update are three device
    kernels inside ``FusedAdamW.step`` (one statistics pass, ``pm_loss_scale_update``, then an AdamW that multiplies by
    1/scale or returns untouched), so the host never waits.  ``unscale_`` is therefore a no-op kept for call-compatibility:
    the flat gradients stay scaled, ``unscaled_grad_stats`` gives the reference's logged norms.
    torch's own GradScaler also works with these models and FusedAdamW (the backward is linear in the loss gradient)."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, enabled: bool = True):
        self.init_scale, self.growth_factor, self.backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        self.growth_interval, self.enabled = int(growth_interval), bool(enabled)
        self._state: Optional[torch.Tensor] = None   # f32[8] on the device: pm_loss_scale_update's record
        self._stats: Optional[torch.Tensor] = None   # f32[3]: sum g^2, #NaN, #Inf of the last step's scaled gradients
        self._pending: Optional[dict] = None         # a state dict loaded before the device is known

    def _device_state(self, device):
        if self._state is None or self._state.device != torch.device(device):
            st = torch.zeros(8, dtype=torch.float32)
            st[0] = self.init_scale
            if self._pending is not None:
                st[0], st[1] = float(self._pending["scale"]), float(self._pending.get("_growth_tracker", 0))
                self._pending = None
            self._state = st.to(device)
            self._stats = torch.zeros(3, dtype=torch.float32, device=device)
        return self._state, self._stats

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        if not self.enabled:
            return loss
        state, _ = self._device_state(loss.device)
        return _ScaleLossFn.apply(loss, state[0:1])

    def unscale_(self, optimizer) -> None:
        """No-op: FusedAdamW unscales inside its update (see the class comment), so the flat gradients are STILL multiplied by the
        loss scale after this call.  Do not follow it with `torch.nn.utils.clip_grad_norm_`: that would clip scaled gradients
        without any error.  Clip with `scaler.step(optimizer, max_norm=...)` (FusedAdamW.step), which clips the unscaled
        gradient on the device; `optimizer.grad_norms(scaler)` gives the unscaled per-group norms."""

    def step(self, optimizer, *args, **kwargs):
        if not isinstance(optimizer, FusedAdamW):
            raise _lib.PolypMaeError("LossScaler.step needs ssl4polyp_amd.optim.FusedAdamW (the skip / unscale decision runs inside "
                                     "its device kernels); use torch.cuda.amp.GradScaler with other optimizers")
        return optimizer.step(*args, loss_scaler=self if self.enabled else None, **kwargs)

    def update(self, new_scale: Optional[float] = None) -> None:
        """The scale already moved inside step() (device side).  new_scale: set it explicitly, as GradScaler.update does."""
        if new_scale is not None and self._state is not None:
            self._state[0] = float(new_scale)
            self._state[1] = 0.0

    def unscaled_grad_stats(self, optimizer) -> torch.Tensor:
        """[sum(g^2), #NaN, #Inf] of the UNSCALED gradients (device tensor, no host sync): what the reference logs after
        scaler.unscale_ (train_classification.py:4535-4544)."""
        gs = optimizer.grad_stats()
        if self.enabled and self._state is not None:
            gs[0] = gs[0] / (self._state[0] * self._state[0])
        return gs

    # -- host-side views (each is one device read-back: logging / checkpoints only) -------------------------------------------
    def get_scale(self) -> float:
        if not self.enabled:
            return 1.0
        if self._state is None:
            return float(self._pending["scale"]) if self._pending is not None else self.init_scale
        return float(self._state[0])

    def counters(self) -> dict:
        """{"steps", "skipped", "found_inf_last"} since construction."""
        if self._state is None:
            return {"steps": 0, "skipped": 0, "found_inf_last": False}
        v = self._state.tolist()
        return {"steps": int(v[4]), "skipped": int(v[3]), "found_inf_last": bool(v[2])}

    def state_dict(self) -> dict:
        """torch.cuda.amp.GradScaler's layout (what the reference's checkpoints store: misc.py:311-318, tc.py:7036-7067)."""
        if not self.enabled:
            return {}
        tracker = int(self._state[1]) if self._state is not None else int((self._pending or {}).get("_growth_tracker", 0))
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, sd: dict) -> None:
        if not sd:
            return
        self.growth_factor = float(sd.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(sd.get("backoff_factor", self.backoff_factor))
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
        if self._state is not None:
            self._state[0] = float(sd["scale"])
            self._state[1] = float(sd.get("_growth_tracker", 0))
        else:
            self._pending = dict(sd)


class FusedLARS(torch.optim.Optimizer):
    """LARS as the MAE linear probe uses it (mae/util/lars.py: the MoCo v3 implementation), the reference's constructor, one
    `pm_lars_step` call per param group over a table of its tensors: parameters with more than one dimension get weight decay and
    the trust ratio q = tc |p| / |g + wd p| (q = 1 when either norm is 0), the others neither; mu = momentum mu + dp, p -= lr mu.

    The parameters are any contiguous f32 tensors on the GPU (the probe head's two, or views into a model's flat storage).  lr,
    weight decay, momentum and the trust coefficient live in a device record per group that the kernels read: `step()` refreshes
    it from `param_groups` without a host sync (so `lr_sched.adjust_learning_rate`, `lr_scale` included, works unchanged), and
    under stream capture leaves it alone -- call `sync_hyper()` between graph replays.  `state_dict()` has the reference's layout
    (per-parameter `mu`; the groups' lr / weight_decay / momentum / trust_coefficient) and `load_state_dict` accepts the
    reference's."""

    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient)
        super().__init__(params, defaults)
        self._hyper: Optional[torch.Tensor] = None
        self._hyper_host = None
        self._tables: Dict[int, tuple] = {}

    def _rows(self):
        return [(float(g["lr"]), float(g["weight_decay"]), float(g["momentum"]), float(g["trust_coefficient"])) for g in self.param_groups]

    def sync_hyper(self, device=None) -> None:
        """Push the groups' hyper-parameters to the device records when they changed on the host (an asynchronous copy)."""
        rows = self._rows()
        if self._hyper is None or (device is not None and self._hyper.device != torch.device(device)) or \
                self._hyper.shape[0] != len(rows):
            if device is None:
                device = next(p.device for g in self.param_groups for p in g["params"])
            self._hyper = torch.zeros(len(rows), 4, dtype=torch.float32, device=device)
            self._hyper_host = None
        if rows != self._hyper_host:
            self._hyper.copy_(torch.tensor(rows, dtype=torch.float32).pin_memory(), non_blocking=True)
            self._hyper_host = rows

    def _table(self, gi: int, group):
        """(pm_lars_segment array, workspace) of the group's parameters that have a gradient; rebuilt when a buffer moved."""
        live = [p for p in group["params"] if p.grad is not None]
        for p in live:
            if p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                raise _lib.PolypMaeError("FusedLARS: parameters must be contiguous f32 tensors on the GPU")
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != p.device:
                raise _lib.PolypMaeError("FusedLARS: gradients must be contiguous f32 tensors on the parameter's device")
            if "mu" not in self.state[p]:
                self.state[p]["mu"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["mu"].data_ptr(), p.numel(), p.ndim > 1) for p in live)
        cached = self._tables.get(gi)
        if cached is None or cached[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.PolypMaeError("FusedLARS: the set of gradients changed under stream capture; take one eager step first")
            arr = (_lib.LarsSegment * max(len(key), 1))()
            for i, (pp, gp, mp, n, mat) in enumerate(key):
                arr[i] = _lib.LarsSegment(pp, gp, mp, n, 1 if mat else 0)
            ws = (torch.empty(max(_lib.workspace_bytes("pm_lars_workspace", len(key)) // 8, 1), dtype=torch.float64, device=live[0].device)
                  if key else None)
            cached = self._tables[gi] = (key, arr, ws)
        return cached

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing() and self._hyper is not None):
            self.sync_hyper()
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            key, arr, ws = self._table(gi, group)
            if not key:
                continue
            _lib.check(lib.pm_lars_step(arr, len(key), _ptr(self._hyper[gi]), _ptr(ws), ws.numel() * 8, _stream()), "pm_lars_step")
        return loss
