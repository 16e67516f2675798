"""Cohort plan of FusedAdamW(per_parameter_steps=True): pure host arithmetic, no torch, no device.

torch.optim.AdamW keeps ``state[p]["step"]`` per parameter: a parameter's step counts the optimizer steps in which it had a gradient
(torch/optim/adamw.py: parameters with ``p.grad is None`` are left out of the step, and their state is created at their first one).
The fused optimizer keeps its step in a 16-float device record that the update kernel reads by pointer, so the unit that can have a
step of its own is a record.  A COHORT is the set of a param group's parameters that share one step history, and therefore one
record.  The plan follows the ``p.grad is None`` pattern from step to step:

  * a parameter that has a gradient for the first time joins a new cohort at step 0 (it is ticked to 1 by the same step);
  * a cohort of which only a part has a gradient this step splits: the part WITHOUT a gradient moves to a new record that starts
    as a copy of the old one (its step and moments stay; it continues from there when it is trainable again);
  * only the records with a gradient this step are ticked;
  * a parameter that never had a gradient has no cohort, as torch holds no state for it.

Records [0, G) are the first cohort of each of the G param groups (so a run whose pattern never changes has R == G records, record g
= group g, exactly the default optimizer's layout); later records are appended.  Cohorts are never merged while a run lasts: two
cohorts whose step counts happen to agree simply stay two records.  `from_steps` (load_state_dict) does group equal steps together,
which is safe because the next `advance` splits them again wherever their patterns differ.
"""
from __future__ import annotations

from typing import Dict, Hashable, Iterable, List, Optional, Sequence, Tuple


class CohortPlan:
    """group_of[r]: the param group of record r.  steps[r]: HOST mirror of record r's step (every call of `advance` counts; the
    device record is authoritative, because a step skipped by the loss scaler does not count there).  cohort[key]: the record of a
    parameter, absent while it was never updated.  Keys are whatever hashable names the caller gives its parameters."""

    def __init__(self, n_groups: int):
        if n_groups <= 0:
            raise ValueError("CohortPlan needs at least one param group")
        self.n_groups = int(n_groups)
        self.group_of: List[int] = list(range(self.n_groups))
        self.steps: List[int] = [0] * self.n_groups
        self.cohort: Dict[Hashable, int] = {}
        self._base_used: List[bool] = [False] * self.n_groups

    @property
    def n_records(self) -> int:
        return len(self.group_of)

    def _new_record(self, group: int, step: int) -> int:
        if not self._base_used[group]:
            self._base_used[group] = True
            self.steps[group] = int(step)
            return group
        self.group_of.append(group)
        self.steps.append(int(step))
        return len(self.group_of) - 1

    def preview(self, groups: Sequence[Sequence[Hashable]], active) -> bool:
        """True when `advance(groups, active)` would create or split a cohort (a captured step cannot follow that)."""
        active = set(active)
        for keys in groups:
            seen: Dict[int, List[bool]] = {}
            for k in keys:
                r = self.cohort.get(k)
                if r is None:
                    if k in active:
                        return True
                else:
                    seen.setdefault(r, [False, False])[0 if k in active else 1] = True
            if any(a and b for a, b in seen.values()):
                return True
        return False

    def advance(self, groups: Sequence[Sequence[Hashable]], active) -> Tuple[List[Tuple[int, int]], List[int]]:
        """One optimizer step in which exactly the parameters in `active` have a gradient.  groups: the keys of every param group,
        in group order.  Returns (copies, tick): copies = [(new record, the record it starts as a copy of)] for the splits of this
        step, in the order they must be applied; tick = the records to advance, ascending.  The host mirrors of `tick` advance."""
        active = set(active)
        copies: List[Tuple[int, int]] = []
        tick = set()
        for gi, keys in enumerate(groups):
            members: Dict[int, Tuple[List[Hashable], List[Hashable]]] = {}
            fresh: List[Hashable] = []
            for k in keys:
                r = self.cohort.get(k)
                if r is None:
                    if k in active:
                        fresh.append(k)
                    continue
                if self.group_of[r] != gi:
                    raise ValueError(f"parameter {k!r} moved from param group {self.group_of[r]} to {gi}")
                members.setdefault(r, ([], []))[0 if k in active else 1].append(k)
            for r in sorted(members):
                act, idle = members[r]
                if act and idle:   # split: the idle part keeps its history in a record of its own
                    r2 = self._new_record(gi, self.steps[r])
                    copies.append((r2, r))
                    for k in idle:
                        self.cohort[k] = r2
                if act:
                    tick.add(r)
            if fresh:
                r = self._new_record(gi, 0)
                for k in fresh:
                    self.cohort[k] = r
                tick.add(r)
        order = sorted(tick)
        for r in order:
            self.steps[r] += 1
        return copies, order

    def records_of(self, groups: Sequence[Sequence[Hashable]], active) -> List[Dict[int, List[Hashable]]]:
        """Per param group {record: its parameters in `active`, in group order}: the segment -> record map of a step (call after
        `advance`, when every active parameter has a cohort)."""
        active = set(active)
        out = []
        for keys in groups:
            by: Dict[int, List[Hashable]] = {}
            for k in keys:
                if k in active:
                    by.setdefault(self.cohort[k], []).append(k)
            out.append(by)
        return out

    def parameter_steps(self, record_steps: Optional[Sequence[float]] = None) -> Dict[Hashable, int]:
        """{key: step} of every parameter with a cohort, from `record_steps` (the device records' slot [6], read at checkpoint time)
        or from the host mirrors.  A parameter whose record is still at step 0 -- its only steps were skipped by the loss scaler --
        is left out: torch's GradScaler never called optimizer.step() for it, so torch holds no state either."""
        src = self.steps if record_steps is None else record_steps
        out = {}
        for k, r in self.cohort.items():
            s = int(round(float(src[r])))
            if s > 0:
                out[k] = s
        return out

    @classmethod
    def from_steps(cls, groups: Sequence[Sequence[Hashable]], steps: Dict[Hashable, float]) -> "CohortPlan":
        """The plan of a loaded state dict: per param group, the parameters that have an entry form one cohort per distinct step (in
        order of first appearance); parameters without an entry have none."""
        plan = cls(len(groups))
        for gi, keys in enumerate(groups):
            by_step: Dict[int, int] = {}
            for k in keys:
                if k not in steps:
                    continue
                s = int(round(float(steps[k])))
                if s not in by_step:
                    by_step[s] = plan._new_record(gi, s)
                plan.cohort[k] = by_step[s]
        return plan

    def snapshot(self):
        return list(self.steps)

    def restore(self, snap) -> None:
        self.steps[:len(snap)] = list(snap)


def torch_layout(groups: Sequence[Sequence[Hashable]], steps: Dict[Hashable, int]) -> Tuple[List[List[int]], Dict[int, int]]:
    """torch.optim.Optimizer.state_dict()'s numbering: parameters are numbered 0, 1, ... through the groups in order; returns
    (the id lists of param_groups[*]["params"], {id: step} for the parameters in `steps` only)."""
    ids, state, k = [], {}, 0
    for keys in groups:
        row = []
        for key in keys:
            if key in steps:
                state[k] = steps[key]
            row.append(k)
            k += 1
        ids.append(row)
    return ids, state
