"""Staged fine-tuning on the device: FusedAdamW(per_parameter_steps=True) against torch.optim.AdamW through unfreeze / re-freeze
schedules (the trajectory test fails without the feature), bit-identity with the default optimizer where the gradient pattern never
changes, the new C entry points (tick over a list, clip over cohort records) with their refusals, graphs, forced sync, resume, and
main_finetune end to end.  The model is the suite's tiny classifier (embed 64, depth 3, 2 heads, cls token): the smallest that has a
head, a top block and blocks below it; B = 4 at 224^2; two groups with different lrs, weight decay 0.05."""
import ctypes
import json
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from ssl4polyp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCHEDULE = ["none", "none", "head+1", "head+1", "head+2", "head+2", "head+1", "head+1", "full", "full"]
INIT_SCALE = 4096.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _tiny_cls(prec="fp32", seed=5):
    import ssl4polyp_amd as A
    torch.manual_seed(seed)
    return A.ViT_from_MAE(None, True, 2, False, None, embed_dim=64, depth=3, num_heads=2, out_token="cls", precision=prec).to(DEV)


def _groups(m):
    """Every parameter, frozen ones included (tc.py:5751-5768): head / backbone with different lrs."""
    head = list(m.lin_head.parameters())
    hid = {id(p) for p in head}
    return [{"params": head, "lr": 2e-3, "name": "head"}, {"params": [p for p in m.parameters() if id(p) not in hid], "name": "backbone"}]


def _batch(seed=3):
    imgs = torch.randn(4, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    return imgs, torch.tensor([0, 1, 1, 0], device=DEV)


def _pw():
    """pos_weight as a device scalar (a host float would be uploaded inside the step, which a capture does not allow)."""
    return torch.ones((), dtype=torch.float32, device=DEV)


def _fused(m, **kw):
    from ssl4polyp_amd.optim import FusedAdamW
    return FusedAdamW(m, _groups(m), lr=1e-3, weight_decay=0.05, **kw)


def _buffers(m, opt):
    opt.sync()
    torch.cuda.synchronize()
    f = m._rt.flat
    out = {"P" + r: t.clone() for r, t in f.P.items()}
    out.update({"M" + r: t.clone() for r, t in opt._M.items()})
    out.update({"V" + r: t.clone() for r, t in opt._V.items()})
    if f.S is not None:
        out["S"] = f.S.clone()
    return out


def _names_in_group_order(m, opt):
    """The parameter names in torch's state-dict numbering: through the param groups in order."""
    name = {id(p): n for n, p in m.named_parameters()}
    return [name[id(p)] for g in opt.param_groups for p in g["params"]]


def _steps_of(sd):
    return {k: float(v["step"]) for k, v in sd["state"].items()}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the trajectory against torch.optim.AdamW
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_trajectory_through_unfreeze_and_refreeze_against_torch_adamw(prec):
    """A second engine model is driven by torch.optim.AdamW (fp16: through torch.amp.GradScaler); its weights are set to this
    model's before every step, so both see the same gradients bit for bit (asserted) and every step's update is compared.  fp16: an
    Inf is planted in a gradient on the first step after the first unfreeze -- nothing is touched and the new cohort's step stays 0
    on both sides (torch holds no state for it, this optimizer writes no entry)."""
    import ssl4polyp_amd as A
    from ssl4polyp_amd import train as T
    from ssl4polyp_amd.optim import LossScaler
    imgs, labels = _batch()
    m, ref = _tiny_cls(prec, seed=11), _tiny_cls(prec, seed=11)
    opt = _fused(m, per_parameter_steps=True)
    topt = torch.optim.AdamW(_groups(ref), lr=1e-3, weight_decay=0.05)
    scaled = prec == "fp16"
    sc = LossScaler(init_scale=INIT_SCALE) if scaled else None
    tsc = torch.amp.GradScaler("cuda", init_scale=INIT_SCALE) if scaled else None
    names = _names_in_group_order(m, opt)
    plant_at = SCHEDULE.index("head+1") if scaled else -1
    worst, mode = 0.0, None
    for it, want_mode in enumerate(SCHEDULE):
        if want_mode != mode:
            mode = want_mode
            T.configure_finetune_parameters(m, mode)
            T.configure_finetune_parameters(ref, mode)
        opt.zero_grad(set_to_none=True)
        topt.zero_grad(set_to_none=True)
        loss = A.supervised_loss(m(imgs), labels, pos_weight=_pw())
        tloss = A.supervised_loss(ref(imgs), labels, pos_weight=_pw())
        if scaled:
            sc.scale(loss).backward()
            tsc.scale(tloss).backward()
        else:
            loss.backward()
            tloss.backward()
        updated = []
        for (n, p), q in zip(m.named_parameters(), ref.parameters()):
            assert (p.grad is None) == (q.grad is None), (it, n)
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), (it, n)
                updated.append(n)
        if it == plant_at:   # (after the comparison: every gradient of this step was equal before the Inf went in)
            m.blocks[2].mlp.fc1.weight.grad.view(-1)[1] = float("inf")
            ref.blocks[2].mlp.fc1.weight.grad.view(-1)[1] = float("inf")
        assert updated and (mode == "none") == all(n.startswith("lin_head") for n in updated)
        before = _buffers(m, opt) if it == plant_at else None
        if scaled:
            sc.step(opt)
            sc.update()
            tsc.step(topt)
            tsc.update()
            assert sc.get_scale() == tsc.get_scale() == (INIT_SCALE if it < plant_at else INIT_SCALE / 2)
        else:
            opt.step()
            topt.step()
        if before is not None:
            after = _buffers(m, opt)
            assert all(torch.equal(before[k], after[k]) for k in before)           # the skipped step touched nothing
        with torch.no_grad():
            for (n, p), q in zip(m.named_parameters(), ref.parameters()):
                if n in updated and not n.endswith("attn.qkv.bias"):   # (see test_fused_adamw_matches_torch_adamw_and_graph_replay)
                    e = rel_l2(p, q)
                    worst = max(worst, e)
                    assert e < 2e-5, (it, mode, n, e)
                q.copy_(p)
        # every state_dict() step equals torch's integer exactly; the set of parameters with state equals torch's
        mine, theirs = _steps_of(opt.state_dict()), _steps_of(topt.state_dict())
        assert mine == theirs, (it, mode)
        if it == plant_at:
            assert not any(names[k].startswith("blocks.") for k in mine)            # the new cohort: step 0 on both sides, no entry
    print(f"[measured] {prec}: worst parameter rel-L2 against torch over {len(SCHEDULE)} steps {worst:.3e}; "
          f"records {opt._plan_cohorts().n_records}, device steps {opt._hyper[:, 6].tolist()}")
    skipped = 1 if scaled else 0
    by_name = {names[k]: s for k, s in mine.items()}
    assert by_name["lin_head.weight"] == 10 - skipped and by_name["blocks.2.attn.proj.weight"] == 8 - skipped
    assert by_name["blocks.1.attn.proj.weight"] == 4 and by_name["blocks.0.attn.proj.weight"] == 2 and by_name["cls_token"] == 2
    assert opt._plan_cohorts().n_records <= 2 + len(set(SCHEDULE))
    # the moments at the end
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert set(sd["state"]) == set(tsd["state"]) and len(sd["state"]) > 40
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in tsd["param_groups"]]
    for k in sd["state"]:
        if not names[k].endswith("attn.qkv.bias"):
            for key in ("exp_avg", "exp_avg_sq"):
                assert rel_l2(sd["state"][k][key], tsd["state"][k][key]) < 2e-5, (names[k], key)
    assert names == _names_in_group_order(ref, topt)          # both optimizers number the parameters alike


# ---------------------------------------------------------------------------------------------------------------------------
# 2. no flip, same bits as the default optimizer
# ---------------------------------------------------------------------------------------------------------------------------
def _constant_run(flag, mode, variant, steps=4):
    import ssl4polyp_amd as A
    from ssl4polyp_amd import train as T
    from ssl4polyp_amd.graph import GraphedStep
    from ssl4polyp_amd.optim import LossScaler
    imgs, labels = _batch(7)
    pw = _pw()
    m = _tiny_cls("fp16" if variant == "scaler" else "bf16", seed=3)
    T.configure_finetune_parameters(m, mode)
    opt = _fused(m, per_parameter_steps=flag, overlap_forward=variant == "overlap")
    sc = LossScaler(init_scale=INIT_SCALE) if variant == "scaler" else None
    kw = {"max_norm": 0.01} if variant == "clip" else {}
    norms = []

    def step():
        opt.zero_grad(set_to_none=True)
        loss = A.supervised_loss(m(imgs), labels, pos_weight=pw)
        if sc is not None:
            sc.scale(loss).backward()
            norms.append(opt.grad_norms(sc))
            sc.step(opt)
            sc.update()
        else:
            loss.backward()
            if variant != "graph":
                norms.append(opt.grad_norms())
            opt.step(**kw)
        return loss

    if variant == "graph":
        gs = GraphedStep(step, opt, warmup=1)
        for _ in range(steps - 1):
            gs.replay()
    else:
        for _ in range(steps):
            step()
    out = _buffers(m, opt)
    if norms:
        out["norms"] = torch.stack(norms)
    if variant == "clip":
        out["clip"] = opt.last_clip.clone()
    out["steps"] = torch.tensor(sorted(_steps_of(opt.state_dict()).items()))
    return out, opt


@pytest.mark.parametrize("mode", ["full", "head+2"])
@pytest.mark.parametrize("variant", ["eager", "overlap", "clip", "scaler", "graph"])
def test_constant_mode_gives_the_default_optimizers_bits(mode, variant):
    a, _ = _constant_run(False, mode, variant)
    b, opt = _constant_run(True, mode, variant)
    assert opt._plan_cohorts().n_records == 2 and opt._hyper.shape[0] == 2           # R == G: the default layout
    assert set(a) == set(b) and "S" in a
    for k in a:
        if k == "steps":   # the default writes an entry (its group's step) for never-updated parameters too; the flag does not
            assert set(map(tuple, b[k].tolist())) <= set(map(tuple, a[k].tolist())) and bool((b[k][:, 1] == 4).all())
            # (in "full" that is decoder_pos_embed alone, which the classifier never uses; in "head+2" everything below block 1)
            params = [p for g in opt.param_groups for p in g["params"]]
            assert len(a[k]) == len(params) and len(b[k]) == sum(p.grad is not None for p in params) < len(params)
        else:
            assert torch.equal(a[k], b[k]), (mode, variant, k)
    if variant == "clip":
        assert float(b["clip"][-2]) < 1.0 and b["clip"].shape == (5,)                # the clip was active; [G + 3]
    if "norms" in b:
        assert b["norms"].shape == (4, 3) and bool((b["norms"][:, 2] > 0).all())     # [G + 1]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the new entry points
# ---------------------------------------------------------------------------------------------------------------------------
def _records(R, steps, skip=()):
    h = torch.zeros(R, 16, device=DEV)
    h[:, :6] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0], device=DEV)
    h[:, 6] = torch.tensor([float(s) for s in steps], device=DEV)
    h[:, 11:] = 77.0
    for r in skip:
        h[r, 9] = 1.0
    return h


def _ints(values):
    host = (ctypes.c_int * max(len(values), 1))(*values)
    return torch.tensor(list(values) or [0], dtype=torch.int32, device=DEV), host


def test_tick_over_a_list_gives_the_bits_of_the_tick_over_groups_and_honours_skip():
    lib = _lib.load()
    steps = [0, 3, 9, 1000, 41, 7]
    listed = [0, 2, 3, 5]
    a, b = _records(6, steps, skip=(3,)), _records(6, steps, skip=(3,))
    start = a.clone()
    _lib.check(lib.pm_adamw_tick(a.data_ptr(), 6, _stream()), "pm_adamw_tick")
    dev, host = _ints(listed)
    _lib.check(lib.pm_adamw_tick_list(b.data_ptr(), 6, dev.data_ptr(), host, len(listed), _stream()), "pm_adamw_tick_list")
    torch.cuda.synchronize()
    for r in range(6):
        if r in listed:
            assert torch.equal(a[r], b[r]), r                 # the same f64 pow / sqrt: a cohort at step t = a group at step t
        else:
            assert torch.equal(b[r], start[r]), r             # not named: not touched
    assert torch.equal(b[3], start[3]) and float(b[0, 6]) == 1.0 and float(b[2, 6]) == 10.0
    beta1 = float(torch.tensor(0.9, dtype=torch.float32))     # the record holds f32 values; the arithmetic is f64
    assert float(b[0, 7]) == float(torch.tensor(1.0 - beta1, dtype=torch.float64).float())


def test_refusals_leave_everything_untouched():
    lib = _lib.load()
    h = _records(2, [4, 4])
    before = h.clone()
    good_dev, good = _ints([0, 1])
    for values in ([0, 2], [-1, 1], [1, 1], [1, 0]):                          # outside [0, R), not strictly ascending
        dev, host = _ints(values)
        assert lib.pm_adamw_tick_list(h.data_ptr(), 2, dev.data_ptr(), host, 2, _stream()) == _lib.PM_EINVAL
        assert lib.pm_adamw_segments_list(None, 1, h.data_ptr(), 2, dev.data_ptr(), host, 2, None, _stream(), 0) == _lib.PM_EINVAL
    assert lib.pm_adamw_tick_list(h.data_ptr(), 2, None, good, 2, _stream()) == _lib.PM_EINVAL            # a NULL list
    assert lib.pm_adamw_tick_list(h.data_ptr(), 2, good_dev.data_ptr(), None, 2, _stream()) == _lib.PM_EINVAL
    assert lib.pm_adamw_tick_list(None, 2, good_dev.data_ptr(), good, 2, _stream()) == _lib.PM_EINVAL
    assert lib.pm_adamw_tick_list(h.data_ptr(), 2, good_dev.data_ptr(), good, 3, _stream()) == _lib.PM_ESHAPE
    assert lib.pm_adamw_tick_list(h.data_ptr(), 2, good_dev.data_ptr(), good, 0, _stream()) == _lib.PM_ESHAPE
    # the overlapped sibling: a bad list, a NULL list and a segment whose record is not one of the array's, before any enqueue
    p, g, mm, v = (torch.ones(8, device=DEV) for _ in range(4))
    keep = [t.clone() for t in (p, mm, v)]
    foreign = torch.zeros(16, device=DEV)
    for hyper_ptr, dev, host, want in ((h[1].data_ptr(), None, good, _lib.PM_EINVAL), (foreign.data_ptr(), good_dev, good, _lib.PM_EINVAL),
                                       (h[0].data_ptr() + 4, good_dev, good, _lib.PM_EINVAL)):
        seg = (_lib.AdamwSegment * 1)(_lib.AdamwSegment(p.data_ptr(), g.data_ptr(), mm.data_ptr(), v.data_ptr(), None, 0, 8, hyper_ptr, None))
        got = lib.pm_adamw_segments_list(seg, 1, h.data_ptr(), 2, dev.data_ptr() if dev is not None else None, host, 2, None, _stream(), 0)
        assert got == want
    sumsq = torch.ones(2, dtype=torch.float64, device=DEV)
    record = torch.full((5,), -5.0, dtype=torch.float64, device=DEV)
    for values in ([0, 2], [-1, 0]):                                          # a record of no group
        dev, host = _ints(values)
        assert lib.pm_grad_clip_cohorts(sumsq.data_ptr(), h.data_ptr(), 2, dev.data_ptr(), host, 2, 1.0, 1, 0, record.data_ptr(),
                                        _stream()) == _lib.PM_EINVAL
    assert lib.pm_grad_clip_cohorts(sumsq.data_ptr(), h.data_ptr(), 2, None, good, 2, 1.0, 1, 0, record.data_ptr(), _stream()) == _lib.PM_EINVAL
    assert lib.pm_grad_clip_cohorts(sumsq.data_ptr(), h.data_ptr(), 2, good_dev.data_ptr(), good, 2, 0.0, 1, 0, record.data_ptr(),
                                    _stream()) == _lib.PM_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(h, before) and bool((record == -5.0).all())
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, mm, v)))


def test_a_schedule_on_an_optimizer_with_the_flag_off_is_refused():
    from ssl4polyp_amd import train as T
    m = _tiny_cls("bf16")
    stages = T.materialize_finetune_schedule([{"mode": "none", "epochs": 1}, {"mode": "head+1", "epochs": 1}], 1e-3)
    with pytest.raises(ValueError, match="per_parameter_steps"):
        T.FinetuneScheduleRuntime(stages).apply_if_needed(m, _fused(m), 1)
    opt = _fused(m, per_parameter_steps=True)
    assert T.FinetuneScheduleRuntime(stages).apply_if_needed(m, opt, 1).mode == "none"
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 0.0]


@pytest.mark.parametrize("scaled", [0, 1])
def test_clip_over_cohorts_identity_map_is_pm_grad_clip_bit_for_bit(scaled):
    lib = _lib.load()
    inv = 1.0 / 1024.0
    for sumsq, max_norm, clip in (([1.0, 4.0, 0.0], 10.0, 1), ([1.0, 4.0, 0.0], 1.0, 1), ([3.3e7, 1.7e-3, 9.1], 0.37, 1),
                                  ([2.0, 0.5, 7.0], 1.0, 0), ([float("inf"), 1.0, 1.0], 1.0, 1), ([1e300, 0.0, 0.0], 1.0, 1)):
        s = torch.tensor(sumsq, dtype=torch.float64, device=DEV)
        ha, hb = _records(3, [1, 2, 3]), _records(3, [1, 2, 3])
        for h in (ha, hb):
            h[:, 5] = torch.tensor([1.0, 0.5, 0.25], device=DEV)
            h[:, 10] = inv if scaled else 0.37
        ra, rb = (torch.full((6,), -5.0, dtype=torch.float64, device=DEV) for _ in range(2))
        dev, host = _ints([0, 1, 2])
        _lib.check(lib.pm_grad_clip(s.data_ptr(), ha.data_ptr(), 3, max_norm, clip, scaled, ra.data_ptr(), _stream()), "pm_grad_clip")
        _lib.check(lib.pm_grad_clip_cohorts(s.data_ptr(), hb.data_ptr(), 3, dev.data_ptr(), host, 3, max_norm, clip, scaled, rb.data_ptr(),
                                            _stream()), "pm_grad_clip_cohorts")
        torch.cuda.synchronize()
        assert torch.equal(ha, hb) and torch.equal(ra.view(torch.int64), rb.view(torch.int64)), (sumsq, max_norm, clip)


def test_clip_over_cohorts_sums_a_groups_records_in_ascending_order():
    lib = _lib.load()
    sumsq = [1.0, 4.0, 1e-17, 0.25, 2.0]                    # records; the map: groups 0, 1, 0, 2(empty: none), 1 -> G = 3
    group_of = [0, 1, 0, 1, 1]
    s = torch.tensor(sumsq, dtype=torch.float64, device=DEV)
    h = _records(5, [1, 1, 1, 1, 1])
    h[:, 5] = 0.5
    before = h.clone()
    rec = torch.full((6,), -5.0, dtype=torch.float64, device=DEV)
    dev, host = _ints(group_of)
    _lib.check(lib.pm_grad_clip_cohorts(s.data_ptr(), h.data_ptr(), 5, dev.data_ptr(), host, 3, 0.5, 1, 0, rec.data_ptr(), _stream()),
               "pm_grad_clip_cohorts")
    torch.cuda.synchronize()
    g0, g1 = (1.0 + 1e-17), ((4.0 + 0.25) + 2.0)
    total = math.sqrt(g0 * 0.25 + g1 * 0.25)
    coef = min(1.0, 0.5 / (total + 1e-6))
    got = rec.tolist()
    assert got[0] == math.sqrt(g0) * 0.5 and got[1] == math.sqrt(g1) * 0.5 and got[2] == 0.0
    assert abs(got[3] - total) <= 1e-15 * total and abs(got[4] - coef) <= 1e-15 * coef and got[5] == 0.5
    other = [c for c in range(16) if c != 10]
    assert torch.equal(h[:, other], before[:, other])
    assert h[:, 10].tolist() == [float(torch.tensor(coef, dtype=torch.float64).float())] * 5      # into all R records


# ---------------------------------------------------------------------------------------------------------------------------
# 4. clipped, mid-schedule
# ---------------------------------------------------------------------------------------------------------------------------
def test_clipped_step_across_an_unfreeze_against_clip_grad_norm_and_torch_adamw():
    import ssl4polyp_amd as A
    from ssl4polyp_amd import train as T
    imgs, labels = _batch()
    MAX_NORM = 0.01
    m, ref = _tiny_cls("fp32", seed=11), _tiny_cls("fp32", seed=11)
    opt = _fused(m, per_parameter_steps=True)
    topt = torch.optim.AdamW(_groups(ref), lr=1e-3, weight_decay=0.05)
    mode = None
    for it, want_mode in enumerate(["none", "head+1", "head+1", "head+2", "head+1", "full"]):
        if want_mode != mode:
            mode = want_mode
            T.configure_finetune_parameters(m, mode)
            T.configure_finetune_parameters(ref, mode)
        opt.zero_grad(set_to_none=True)
        topt.zero_grad(set_to_none=True)
        A.supervised_loss(m(imgs), labels, pos_weight=_pw()).backward()
        A.supervised_loss(ref(imgs), labels, pos_weight=_pw()).backward()
        gn = [math.sqrt(sum(float(p.grad.double().square().sum()) for p in g["params"] if p.grad is not None)) for g in opt.param_groups]
        total = math.sqrt(sum(v * v for v in gn))
        pre = opt.grad_norms().cpu().numpy()
        total_t = float(torch.nn.utils.clip_grad_norm_([p for g in topt.param_groups for p in g["params"] if p.grad is not None], MAX_NORM))
        opt.step(max_norm=MAX_NORM)
        topt.step()
        rec = opt.last_clip.cpu().numpy()
        coef = min(1.0, MAX_NORM / (total + 1e-6))
        print(f"[measured] step {it} ({mode}): last_clip {rec.tolist()}; float64 groups {gn}, total {total}, coef {coef}; torch {total_t}")
        assert rec.shape == (5,) and pre.shape == (3,) and total > MAX_NORM
        for g in range(2):
            assert abs(rec[g] - gn[g]) <= 1e-12 * gn[g] and abs(pre[g] - gn[g]) <= 1e-12 * gn[g]
        assert abs(rec[2] - total) <= 1e-12 * total and abs(pre[2] - total) <= 1e-12 * total and abs(rec[3] - coef) <= 1e-12 * coef
        assert rec[4] == MAX_NORM and abs(rec[2] - total_t) < 1e-5 * total_t
        with torch.no_grad():
            for (n, p), q in zip(m.named_parameters(), ref.parameters()):
                if p.grad is not None and not n.endswith("attn.qkv.bias"):
                    assert rel_l2(p, q) < 2e-5, (it, n)
                q.copy_(p)
        assert _steps_of(opt.state_dict()) == _steps_of(topt.state_dict())
    assert opt._plan_cohorts().n_records == 4 and float(opt._hyper[:, 10].min()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 5. graph, forced sync, resume
# ---------------------------------------------------------------------------------------------------------------------------
STAGES = [("none", 2), ("head+1", 2), ("full", 2)]


def _staged_run(graph, overlap=False, ddp_force=None, upto=None, resume=None):
    import ssl4polyp_amd as A
    from ssl4polyp_amd import train as T
    from ssl4polyp_amd.graph import GraphedStep
    imgs, labels = _batch(9)
    pw = _pw()
    m = _tiny_cls("bf16", seed=7)
    fwd = m
    opt = _fused(m, per_parameter_steps=True, overlap_forward=overlap)
    if ddp_force is not None:
        from ssl4polyp_amd.parallel import DataParallel
        fwd = DataParallel(m, torch.device("cuda", 0), bucket_mb=0.05, force_sync=ddp_force)
        if ddp_force:
            opt.grad_sync = fwd.sync
    if resume is not None:
        m.load_state_dict(resume["model"])
        m._rt.ensure(torch.device("cuda", 0))
        opt.load_state_dict(resume["optimizer"])

    def step():
        opt.zero_grad(set_to_none=True)
        loss = A.supervised_loss(fwd(imgs), labels, pos_weight=pw)
        loss.backward()
        opt.step()
        return loss

    done, saved = 0, None
    for mode, n in STAGES:
        first = done
        done += n
        if resume is not None and done <= resume["step"]:
            continue
        T.configure_finetune_parameters(m, mode)
        todo = done - max(first, resume["step"] if resume is not None else 0)
        if graph:
            gs = GraphedStep(step, opt, warmup=1)          # one capture per stage: the plan is fixed while a graph lives
            for _ in range(todo - 1):
                gs.replay()
        else:
            for k in range(todo):
                step()
                if upto is not None and done - todo + k + 1 == upto:
                    opt.sync()
                    saved = {"model": {k2: v.clone() for k2, v in m.state_dict().items()}, "optimizer": opt.state_dict(), "step": upto}
    out = _buffers(m, opt)
    out["steps"] = torch.tensor(sorted(_steps_of(opt.state_dict()).items()))
    return out, saved, m


def test_one_graph_per_stage_replays_the_eager_trajectory_bit_for_bit():
    eager, _, _ = _staged_run(False)
    graph, _, _ = _staged_run(True)
    assert sorted(set(eager["steps"][:, 1].tolist())) == [2.0, 4.0, 6.0]
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    # the plan cannot follow a changed pattern inside a capture: a refusal, not a wrong update
    from ssl4polyp_amd import train as T
    from ssl4polyp_amd.graph import GraphedStep
    import ssl4polyp_amd as A
    imgs, labels = _batch(9)
    pw = _pw()
    m = _tiny_cls("bf16", seed=7)
    opt = _fused(m, per_parameter_steps=True)
    T.configure_finetune_parameters(m, "none")
    calls = {"n": 0}

    def step():
        calls["n"] += 1
        if calls["n"] == 2:                                  # the captured call sees another pattern than the warm-up did
            T.configure_finetune_parameters(m, "head+1")
        opt.zero_grad(set_to_none=True)
        loss = A.supervised_loss(m(imgs), labels, pos_weight=pw)
        loss.backward()
        opt.step()
        return loss
    with pytest.raises(_lib.PolypMaeError, match="fixed while a graph lives"):
        GraphedStep(step, opt, warmup=1)


def test_resume_in_the_second_stage_continues_bit_for_bit_and_loads_into_torch_adamw():
    whole, saved, m = _staged_run(False, upto=3)
    assert saved is not None and sorted(set(_steps_of(saved["optimizer"]).values())) == [1.0, 3.0]
    part, _, _ = _staged_run(False, resume=dict(saved, step=3))
    for k in whole:
        assert torch.equal(whole[k], part[k]), k
    names = _names_in_group_order(m, _fused(m))
    state = saved["optimizer"]["state"]
    assert all(names[k].startswith(("lin_head", "blocks.2.")) for k in state) and len(state) < len(names)   # no entry: never updated
    assert set(saved["optimizer"]["param_groups"][1]) == {"lr", "betas", "eps", "weight_decay", "name", "params"}   # torch's layout
    ref = _tiny_cls("bf16", seed=7)
    topt = torch.optim.AdamW(_groups(ref), lr=1e-3, weight_decay=0.05)
    topt.load_state_dict(saved["optimizer"])
    assert _steps_of(topt.state_dict()) == _steps_of(saved["optimizer"])
    # and the reverse: torch's dict into this optimizer
    other = _fused(ref, per_parameter_steps=True)
    ref._rt.ensure(torch.device("cuda", 0))
    other.load_state_dict(topt.state_dict())
    assert _steps_of(other.state_dict()) == _steps_of(saved["optimizer"])
    assert other._plan_cohorts().steps == [3, 1]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(port, q):
    """world size 1 on the RCCL backend, the synchroniser forced on, overlapped AdamW with per-parameter steps, none -> head+1 ->
    full (the worker pattern of tests/test_gpu_parallel.py)."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        a, _, _ = _staged_run(False, overlap=True, ddp_force=True)
        b, _, _ = _staged_run(False, overlap=True, ddp_force=False)
        c, _, _ = _staged_run(False)
        q.put((all(torch.equal(a[k], b[k]) for k in a), all(torch.equal(a[k], c[k]) for k in a), a["steps"][:, 1].tolist()))
    finally:
        dist.destroy_process_group()


def test_world1_forced_sync_with_overlapped_update_matches_unsynchronised_run():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_sync_worker, args=(_free_port(), q))
    p.start()
    same_sync, same_eager, steps = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert same_sync and same_eager and sorted(set(steps)) == [2.0, 4.0, 6.0]


# ---------------------------------------------------------------------------------------------------------------------------
# 6. main_finetune end to end
# ---------------------------------------------------------------------------------------------------------------------------
def _log(path):
    return [json.loads(ln) for ln in open(path)]


def test_main_finetune_runs_a_schedule_and_stops_early(tmp_path, monkeypatch):
    import csv
    from pack_files import encode, frame
    from ssl4polyp_amd import main_finetune as M
    from ssl4polyp_amd import train as T
    root = tmp_path / "data"
    (root / "img").mkdir(parents=True)
    with open(tmp_path / "train.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame_path", "label", "store_id", "variant"])
        for i in range(8):
            (root / "img" / f"{i:02d}.jpg").write_bytes(encode(frame(64, 64, 300 + i), subsampling=2, quality=90))
            w.writerow([f"img/{i:02d}.jpg", (i // 2) % 2, "frames", "clean"])
    spec = [{"name": "warm", "mode": "none", "epochs": 1, "head_lr": 5e-4}, {"name": "top", "mode": "head+1", "epochs": 2, "head_lr": 5e-4,
                                                                                "backbone_lr": 5e-6}]
    (tmp_path / "schedule.json").write_text(json.dumps(spec))
    common = ["--train_csv", str(tmp_path / "train.csv"), "--val_csv", str(tmp_path / "train.csv"), "--root", f"frames={root}",
              "--batch_size", "4", "--precision", "bf16", "--num_workers", "0", "--no_pin_mem", "--seed", "3", "--epochs", "3",
              "--finetune_schedule", str(tmp_path / "schedule.json")]
    with pytest.raises(SystemExit, match="finetune_mode"):
        M.run(M.get_args_parser().parse_args(common + ["--finetune_mode", "head+2", "--output_dir", str(tmp_path / "bad")]))
    seen = []
    real = M.train_epoch_cls

    def spy(model, *a, **kw):
        seen.append(sorted(n for n, p in T._unwrap(model).named_parameters() if p.requires_grad))
        return real(model, *a, **kw)
    monkeypatch.setattr(M, "train_epoch_cls", spy)
    model, _ = M.run(M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "out")]))
    records = _log(tmp_path / "out" / "log.txt")
    assert len(records) == 3 and len(seen) == 3
    # what the runtime + scheduler give for that spec (the restatement is held to the reference's trace on the CPU)
    toy = torch.nn.Module()
    toy.lin_head, toy.blocks = torch.nn.Linear(2, 2), torch.nn.ModuleList([torch.nn.Linear(2, 2)])
    head = list(toy.lin_head.parameters())
    topt = torch.optim.AdamW([{"params": head, "name": "head"}, {"params": list(toy.blocks.parameters()), "name": "backbone"}], lr=1e-3)
    runtime = T.FinetuneScheduleRuntime(T.materialize_finetune_schedule(spec, 1e-3))
    sched = T.create_scheduler(topt, "cosine", 3, 0)
    for epoch, rec in enumerate(records):
        stage = runtime.apply_if_needed(toy, topt, epoch + 1)
        assert (rec["epoch"], rec["stage"], rec["mode"], rec["lr_groups"]) == (epoch, stage.index, stage.mode, [g["lr"] for g in topt.param_groups])
        topt.step()
        sched.step()
    assert [r["mode"] for r in records] == ["none", "head+1", "head+1"] and records[0]["lr_groups"] == [5e-4, 0.0]
    assert records[1]["lr_groups"] == [5e-4, 5e-6] and records[2]["lr_groups"][0] == records[2]["lr_groups"][1]   # the kept quirk
    names = [n for n, _ in model.named_parameters()]
    stored = [n for n in names if n.startswith("lin_head")] + [n for n in names if not n.startswith("lin_head")]   # head group first
    last = len(model.blocks) - 1
    assert seen[0] == sorted(n for n in names if n.startswith("lin_head"))
    assert seen[1] == seen[2] == sorted(n for n in names if n.startswith(("lin_head", f"blocks.{last}.")))
    ckpt = torch.load(str(tmp_path / "out" / "ckpts" / "finetune_e2.pth"), map_location="cpu", weights_only=False)
    assert ckpt["finetune_stage_index"] == 1 and "scheduler_state_dict" in ckpt
    steps = {stored[k]: float(v["step"]) for k, v in ckpt["optimizer_state_dict"]["state"].items()}
    assert steps["lin_head.weight"] == 2 * steps[f"blocks.{last}.attn.proj.weight"] > 0      # two epochs against one
    assert not any(n.startswith("blocks.0.") for n in steps)
    # resume from the second epoch's checkpoint: the third epoch's record again, in the stage it left
    M.run(M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "again"), "--resume",
                                                   str(tmp_path / "out" / "ckpts" / "finetune_e2.pth")]))
    again, = _log(tmp_path / "again" / "log.txt")
    assert (again["epoch"], again["stage"], again["mode"], again["lr_groups"]) == (2, 1, "head+1", records[2]["lr_groups"])
    assert seen[3] == seen[2]
    # early stopping: min_delta 1e9 lets nothing count as an improvement after the first epoch
    M.run(M.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / "stop"), "--early_stop_patience", "1",
                                                   "--early_stop_min_delta", "1e9"]))
    stopped = _log(tmp_path / "stop" / "log.txt")
    want = next(e for e in range(1, 4) if T.should_trigger_early_stop(e - 1, 1, e, 0))
    assert len(stopped) == want == 2 and [r["stopped"] for r in stopped] == [False, True]
    assert [r["no_improve"] for r in stopped] == [0, 1] and stopped[1]["best"] == stopped[0]["monitor"] == stopped[0]["val_loss"]
    ckpt = torch.load(str(tmp_path / "stop" / "ckpts" / "finetune_e2.pth"), map_location="cpu", weights_only=False)
    assert ckpt["early_stop_state"]["no_improve"] == 1 and ckpt["finetune_stage_index"] == 1
    # --resume of a default run without a val split (its checkpoints carry no monitor value): the optimizer state is restored too
    plain = ["--train_csv", str(tmp_path / "train.csv"), "--root", f"frames={root}", "--batch_size", "4", "--precision", "bf16",
             "--num_workers", "0", "--no_pin_mem", "--seed", "3", "--finetune_mode", "head+1"]
    M.run(M.get_args_parser().parse_args(plain + ["--epochs", "1", "--output_dir", str(tmp_path / "plain")]))
    M.run(M.get_args_parser().parse_args(plain + ["--epochs", "2", "--output_dir", str(tmp_path / "plain2"), "--resume",
                                                  str(tmp_path / "plain" / "ckpts" / "finetune_e1.pth")]))
    first = torch.load(str(tmp_path / "plain" / "ckpts" / "finetune_e1.pth"), map_location="cpu", weights_only=False)
    second = torch.load(str(tmp_path / "plain2" / "ckpts" / "finetune_e2.pth"), map_location="cpu", weights_only=False)
    assert "monitor_value" not in first and "finetune_stage_index" not in first            # the parent's checkpoint keys
    one, two = (float(c["optimizer_state_dict"]["state"][0]["step"]) for c in (first, second))
    assert one > 0 and two == 2 * one and [r["epoch"] for r in _log(tmp_path / "plain2" / "log.txt")] == [1]
