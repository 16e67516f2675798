"""pm_gemm_ex / pm_wgrad_group on every case of tests/gemm_cases.py against the float64 reference and the element-wise bound of
tests/gemm_ref.py (derived from the rounding points, no safety factor; tests/test_gemm_ref_cpu.py), in both operand regimes, with
the old norm-wise bound of tests/test_gpu_ops.py asserted beside it.  Every output (C, the stored pre-activation, the split-K
workspace) lies between guards on all sides: rows in front and behind, and the ldc - N columns to the right of every row; padded
operands carry NaN in their padding and one NaN row behind them, so nothing beyond M / N / K may reach a result.  Then locality
(a NaN row of A / B poisons exactly its row / column of C), invariance (more rows, more columns, padded leading dimensions and a
second run give the same bits), split-K against whole-K, and the refusals.  Each case prints its err / bound (`pytest -s`);
docs/EXPERIMENT_LOG.md has the peaks per family."""
import ctypes

import pytest
import torch

import gemm_cases as G
import gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL, GROWS, GUARD = 7.0, 4, 256   # guard value; guard rows in front of and behind an output (4 rows keep 16-byte alignment)
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def _lib():
    from ssl4polyp_amd import _lib as L
    return L


def _codes():
    L = _lib()
    return ({"bf16": L.PM_BF16, "fp16": L.PM_F16, "fp32": L.PM_F32},
            {"store": L.EPI_STORE, "gelu": L.EPI_GELU, "resid": L.EPI_RESIDUAL, "dgelu": L.EPI_DGELU, "accum": L.EPI_ACCUM})


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _operand(mat, kmajor, pad):
    """The operand as stored ([R][K], or [K][R] when k-major) inside a NaN buffer with `pad` columns to the right of every row and one
    row behind -> (buffer, leading dimension)."""
    m = mat.t() if kmajor else mat
    buf = torch.full((m.shape[0] + 1, m.shape[1] + pad), NAN, dtype=m.dtype, device=DEV)
    buf[:-1, :m.shape[1]] = m
    return buf, m.shape[1] + pad


class Out:
    """An [M][N] output with leading dimension N + pad between guards: GROWS rows in front and behind, the pad columns."""

    def __init__(self, M, N, pad, dtype, init=None, pad_fill=FILL):
        self.M, self.N, self.pad_fill = M, N, pad_fill
        self.buf = torch.full((M + 2 * GROWS, N + pad), FILL, dtype=dtype, device=DEV)
        self.buf[GROWS:GROWS + M, N:] = pad_fill
        self.view = self.buf[GROWS:GROWS + M, :N]
        if init is not None:
            self.view.copy_(init)
        else:
            self.view.fill_(NAN)
        self.ptr = self.buf[GROWS].data_ptr()
        assert self.ptr % 16 == 0

    def guards_hold(self, what):
        assert bool((self.buf[:GROWS] == FILL).all()), what + ": written in front of row 0"
        assert bool((self.buf[GROWS + self.M:] == FILL).all()), what + ": written behind row M"
        pad = self.buf[GROWS:GROWS + self.M, self.N:]
        same = torch.isnan(pad) if self.pad_fill != self.pad_fill else pad == self.pad_fill
        assert bool(same.all()), what + ": written to the right of column N"


def launch(c, o, M=None, N=None, pads=None, ws=None, epi=None, status=0, what=None):
    """One pm_gemm_ex call of case c on the first M rows of o["A"] and the first N rows of o["B"] (default: the case's own).
    -> {"C": tensor, "aux": tensor (GELU)} after the guards were checked; status != 0: the call must return it and write nothing."""
    L = _lib()
    DT, EPI = _codes()
    M, N, K = M or c.M, N or c.N, c.K
    pa, pb, pc = pads if pads is not None else (c.pa, c.pb, c.pc)
    epi = epi or c.epi
    what = what or G.case_id(c)
    akm, bkm = G.a_kmajor(c), G.b_kmajor(c)
    A, lda = _operand(o["A"][:M], akm, pa)
    B, ldb = _operand(o["B"][:N], bkm, pb)
    bias = None
    if c.bias:
        bias = torch.full((N + 4,), NAN, device=DEV)
        bias[:N] = o["bias"][:N]
    base = o["base"][:M, :N]
    C = Out(M, N, pc, R.TORCH[c.c_dt], init=base if epi == "accum" else None)
    aux = resid = None
    if epi == "gelu":
        aux = Out(M, N, pc, R.TORCH[c.in_dt])
    elif epi == "dgelu":
        aux = Out(M, N, pc, R.TORCH[c.in_dt], init=o["pre"][:M, :N], pad_fill=NAN)
    elif epi == "resid":
        resid = Out(M, N, pc, torch.float32, init=base, pad_fill=NAN)
    nws = G.ws_bytes(c._replace(M=M, N=N)) if ws is None else ws
    wsbuf = torch.full((nws + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV) if nws else None
    opts = L.GemmOpts(c.max_blocks, c.variant)
    st = L.load().pm_gemm_ex(A.data_ptr(), lda, int(akm), B.data_ptr(), ldb, int(bkm), DT[c.in_dt],
                             bias.data_ptr() if bias is not None else None, C.ptr, N + pc, DT[c.c_dt], EPI[epi],
                             aux.ptr if aux is not None else None, resid.ptr if resid is not None else None, M, N, K,
                             wsbuf[GUARD:].data_ptr() if nws else None, nws, ctypes.byref(opts), _stream())
    torch.cuda.synchronize()
    assert st == status, f"{what}: status {st}, expected {status}"
    C.guards_hold(what + " C")
    for t, name in ((aux, "aux"), (resid, "resid")):
        if t is not None:
            t.guards_hold(f"{what} {name}")
    if nws:
        assert bool((wsbuf[:GUARD] == 0x5A).all()) and bool((wsbuf[GUARD + nws:] == 0x5A).all()), what + ": written outside the workspace"
    if status:
        assert bool(torch.isnan(C.view).all()) or epi == "accum", what + ": a refused call wrote C"
        return None
    out = {"C": C.view}
    if epi == "gelu":
        out["aux"] = aux.view
    elif epi == "dgelu":
        assert torch.equal(aux.view, o["pre"][:M, :N]), what + ": the saved pre-activation was written"
    elif epi == "resid":
        assert torch.equal(resid.view, base), what + ": the residual input was written"
    return out


_refs = {}


def _reference(M, N, K, dt, regime):
    """(operands on the device, float64 acc, T), made once per shape and never written to."""
    key = (M, N, K, dt, regime)
    if key not in _refs:
        if len(_refs) > 12:
            _refs.clear()
        o = R.operands(M, N, K, dt, regime, DEV)
        _refs[key] = (o,) + R.products(o["A"], o["B"])
    return _refs[key]


def judge(c, o, acc, T, out, what=None, epi=None):
    """Every output of one call against the element-wise bound and the old norm-wise one -> the largest err / bound."""
    what = what or G.case_id(c)
    epi = epi or c.epi
    M, N = out["C"].shape
    exp = R.expected(epi, c.in_dt, c.c_dt, c.K, acc[:M, :N], T[:M, :N], bias=o["bias"][:N] if c.bias else None, base=o["base"][:M, :N],
                     pre=o["pre"][:M, :N], aux_got=out.get("aux"))
    worst = 0.0
    for name, (want, bound, terms) in exp.items():
        ratio, _, text = R.check(out[name], want, bound, terms, f"{what} {name}")
        old, old_bound = R.rel(out[name], want), R.old_bound(c.in_dt, c.in_dt if name == "aux" else c.c_dt, epi, c.K)
        print(f"{text}; norm-wise {old:.3e} (bound {old_bound:.3e})")
        assert ratio < 1.0, text
        assert old < old_bound, f"{text}: norm-wise {old:.3e} >= {old_bound:.3e}"
        worst = max(worst, ratio)
    return worst


def _groups():
    keys = []
    for c in G.CASES:
        k = (c.family, c.cfg if c.family == "ring" else 0, c.in_dt)
        if k not in keys:
            keys.append(k)
    return keys


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("family,cfg,dt", _groups(), ids=lambda v: str(v))
def test_every_case_element_wise(family, cfg, dt, regime):
    """Every case of the table, twice: inside the element-wise bound and the norm-wise one, no guard touched, and the second run
    gives the bits of the first."""
    peak, failed = 0.0, []
    for c in G.CASES:
        if (c.family, c.cfg if c.family == "ring" else 0, c.in_dt) != (family, cfg, dt):
            continue
        o, acc, T = _reference(c.M, c.N, c.K, c.in_dt, regime)
        out = launch(c, o)
        again = launch(c, o)
        try:   # (a case beyond a bound does not hide the cases behind it; a touched guard ends the test at once)
            peak = max(peak, judge(c, o, acc, T, out, f"{regime} {G.case_id(c)}"))
            for name in out:
                assert torch.equal(out[name], again[name]), f"{G.case_id(c)} {name}: a second run gives other bits"
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    print(f"PEAK {regime} {family} cfg {cfg} {dt}: {peak:.3f}")
    assert not failed, "\n".join(failed)


def _group_items(K, dims, dt, regime, with_db):
    items = []
    for j, (n_out, n_in) in enumerate(dims):
        o = R.operands(n_out, n_in, K, dt, regime, DEV)   # A = dY^T [n_out][K], B = X^T [n_in][K]
        acc = j % 2 == 1
        dW = o["base"].clone() if acc else torch.full((n_out, n_in), NAN, device=DEV)
        db = torch.linspace(-1, 1, n_out, device=DEV) if with_db and j != 2 else None
        items.append((o, o["A"].t().contiguous(), o["B"].t().contiguous(), dW, acc, db))
    return items


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("K,dims,dt,with_db", G.GROUP_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else f"{len(v)}problems")
def test_wgrad_group_element_wise(K, dims, dt, with_db, regime):
    """pm_wgrad_group on the scaled operands: every dW inside b_acc element-wise (STORE, and ACCUM on every second problem), the
    bias gradients (db += column sums of dY: exact 16-bit values summed in f32) inside 2 (K + 2) 2^-24 (sum|dY| + |db_in|) of their
    float64 sums; a second run gives the same bits."""
    from ssl4polyp_amd.engine import Kernels
    k = Kernels(dt)
    k.GROUP_MIN_TILES = 0
    runs = []
    for _ in range(2):
        items = _group_items(K, dims, dt, regime, with_db)
        assert k.wgrad_group([(dy, x, dW, acc, db) for _, dy, x, dW, acc, db in items], K)
        torch.cuda.synchronize()
        runs.append(items)
    peak = 0.0
    for j, (o, dy, x, dW, acc, db) in enumerate(runs[0]):
        what = f"{regime} group K={K} {dt} problem {j} {tuple(dW.shape)}"
        a64, T = R.products(o["A"], o["B"])
        exp = R.expected("accum" if acc else "store", dt, "fp32", K, a64, T, base=o["base"] if acc else None)["C"]
        ratio, _, text = R.check(dW, *exp, what)
        old = R.rel(dW, exp[0])
        print(f"{text}; norm-wise {old:.3e}")
        assert ratio < 1.0, text
        assert old < 3e-5 * (K / 32) ** 0.5, text          # (test_wgrad_group's bound)
        peak = max(peak, ratio)
        if db is not None:
            base = torch.linspace(-1, 1, dW.shape[0], device=DEV).double()
            want = base + o["A"].double().sum(1)
            bound = R.b_acc(o["A"].double().abs().sum(1) + base.abs(), K)
            r, _, text = R.check(db[:, None], want[:, None], bound[:, None], {"b_acc": bound[:, None]}, what + " dbias")
            print(text)
            assert r < 1.0, text
        assert torch.equal(dW, runs[1][j][3]) and (db is None or torch.equal(db, runs[1][j][5])), what + ": a second run gives other bits"
    print(f"PEAK {regime} group K={K} {dt}: {peak:.3f}")


@pytest.mark.parametrize("K,slices", [(2080, 1), (8192 + 32, 2)])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wgrad_group_locality_and_invariance(K, slices, dt):
    """Two ragged problems in one group, whole-K (K = 2080) and in two k-slices of 129 + 128 k-steps (K = 8224): each problem
    alone in a group of one plans to the same k-slices and gives the same bits; NaN in one column of a problem's dY (one k index
    of it, in the last slice) makes exactly that row of its dW and that element of its bias gradient non-finite (*), NaN in one
    column of X exactly that column of dW; the other problem keeps its bits.
    (*) The one exemption, by design: the bias gradient is summed on the matrix cores by a 16x16x32 MFMA whose selector operand is 1
    for column r and 0 for column r ^ 16 of the same dY fragment (gemm_v3_tile, XSUM), and 0 x NaN = NaN -- so a non-finite
    dY[:, r] may also make dbias[r ^ 16] non-finite, and nothing else.  With finite gradients the zeros contribute exactly 0; a
    non-finite gradient anywhere makes the loss scaler skip the step as a whole.  Asserted: dbias[r] is non-finite, and no element
    other than r and r ^ 16 is."""
    from ssl4polyp_amd.engine import Kernels
    L = _lib()
    k = Kernels(dt)
    k.GROUP_MIN_TILES = 0
    dims = ((264, 136), (520, 648))
    ops = [R.operands(n_out, n_in, K, dt, "scaled", DEV) for n_out, n_in in dims]

    def run(sel, poison=None):
        items = []
        for j in sel:
            A, B = ops[j]["A"], ops[j]["B"]
            if poison is not None and poison[0] == j:
                A, B = A.clone(), B.clone()
                (A if poison[1] == "dY" else B)[poison[2], K - 5] = NAN
            items.append((A.t().contiguous(), B.t().contiguous(), torch.full(dims[j], NAN, device=DEV), False,
                          torch.zeros(dims[j][0], device=DEV)))
        arr = (L.WgradItem * len(items))()
        for i, (dy, x, dW, _, db) in enumerate(items):
            arr[i] = L.WgradItem(dy.data_ptr(), dW.shape[0], x.data_ptr(), dW.shape[1], dW.data_ptr(), dW.shape[1], dW.shape[0],
                                 dW.shape[1], 0, db.data_ptr())
        got = ctypes.c_int(0)
        assert k.lib.pm_wgrad_group_plan(arr, len(items), K, L.dtype_code(R.TORCH[dt]), None, None, ctypes.byref(got)) == 0
        assert got.value == slices, (sel, got.value)
        assert k.wgrad_group(items, K)
        torch.cuda.synchronize()
        return [(it[2], it[4]) for it in items]

    both = run((0, 1))
    assert all(bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all()) for dW, db in both)
    for j in (0, 1):
        (dW, db), = run((j,))
        assert torch.equal(dW, both[j][0]) and torch.equal(db, both[j][1]), f"problem {j} alone gives other bits than inside the group"
    for j, side, idx in ((0, "dY", 5), (0, "dY", 261), (1, "X", 6), (1, "X", 646), (1, "dY", 517)):
        got = run((0, 1), poison=(j, side, idx))
        other = 1 - j
        assert torch.equal(got[other][0], both[other][0]) and torch.equal(got[other][1], both[other][1]), (j, side, idx)
        bad, bad_b = ~torch.isfinite(got[j][0]), ~torch.isfinite(got[j][1])
        want, want_b, may_b = torch.zeros_like(bad), torch.zeros_like(bad_b), torch.zeros_like(bad_b)
        if side == "dY":
            want[idx] = True
            want_b[idx] = may_b[idx] = True
            if (idx ^ 16) < dims[j][0]:
                may_b[idx ^ 16] = True   # (the partner row of the 16x16x32 MFMA that sums the columns: see the docstring)
        else:
            want[:, idx] = True
        assert torch.equal(bad, want) and bool((bad_b & want_b).sum() == want_b.sum()) and not bool((bad_b & ~may_b).any()), \
            f"NaN in {side}[{idx}] of problem {j}: {int(bad.sum())} non-finite in dW, {bad_b.nonzero().flatten().tolist()} in dbias"


def _representatives():
    """One case per (family, cfg / tile / split-K, layout, operand type) for the locality and invariance tests: for the ring the
    K = 64, N = 264 case of each (cfg, W layout) in bf16 and one in fp16; the 128 x 128 kernels' ragged (129, 132)-like shape per layout
    and operand type; the split-K cases with ragged slices; both weight-gradient tiles."""
    reps, seen = [], set()
    for c in G.CASES:
        if c.family == "ring":
            key = (c.family, c.cfg, c.layout, c.in_dt if c.cfg == 8 else "bf16")
            ok = c.in_dt == key[3] and (c.N, c.K, c.pc) == (264, 64, 0)
        elif c.family == "wgrad":
            key, ok = (c.family, c.tile, c.in_dt == "bf16"), c.in_dt == "bf16" and c.split == 4 and c.variant and c.epi == "store"
        elif c.ws:
            key, ok = (c.family, "splitk", c.in_dt, c.epi), c.split == 5
        else:
            key, ok = (c.family, c.layout, c.in_dt), c.M > 128 and c.N > 128 and c.K > 8
        if ok and key not in seen:
            seen.add(key)
            reps.append(c)
    return reps


REPS = _representatives()


def _poisoned(o, name, row, k=None):
    t = o[name].clone()
    if k is None:
        t[row] = NAN
    else:
        t[row, k] = NAN
    return dict(o, **{name: t})


@pytest.mark.parametrize("c", REPS, ids=G.case_id)
def test_locality(c):
    """NaN in one row r of A makes exactly row r of every output non-finite, NaN in one row n of B exactly column n -- for r / n in
    a full tile and in the ragged last tile; with k-slices, also a single NaN at a k index of the last slice."""
    o = R.operands(c.M, c.N, c.K, c.in_dt, "uniform", DEV)
    rows = sorted({5, c.M - 3})
    cols = sorted({6, c.N - 2})
    probes = [("A", r, None) for r in rows] + [("B", n, None) for n in cols]
    if c.split > 1:
        probes += [("A", rows[-1], c.K - 5), ("B", cols[-1], c.K - 5)]
    for name, idx, k in probes:
        out = launch(c, _poisoned(o, name, idx, k))
        for oname, t in out.items():
            bad = ~torch.isfinite(t)
            want = torch.zeros_like(bad)
            if name == "A":
                want[idx] = True
            else:
                want[:, idx] = True
            assert torch.equal(bad, want), (f"{G.case_id(c)} {oname}: NaN in {name}[{idx}{'' if k is None else ', ' + str(k)}] -> "
                                            f"{int(bad.sum())} non-finite elements, {int((bad & ~want).sum())} outside its row / column, "
                                            f"{int((want & ~bad).sum())} finite inside")


def _plan(c, M, N, pc=0, ws=None):
    L = _lib()
    DT, EPI = _codes()
    opts, info = L.GemmOpts(c.max_blocks, c.variant), L.GemmPlanInfo()
    nws = G.ws_bytes(c._replace(M=M, N=N)) if ws is None else ws
    st = L.load().pm_gemm_plan(int(G.a_kmajor(c)), int(G.b_kmajor(c)), DT[c.in_dt], int(c.bias), DT[c.c_dt], int(pc == 0), EPI[c.epi],
                               M, N, c.K, nws, ctypes.byref(opts), ctypes.byref(info))
    assert st == 0
    return (info.family, info.cfg, info.tile_m, info.tile_n, info.split_k, info.band)


@pytest.mark.parametrize("c", REPS, ids=G.case_id)
def test_invariance(c):
    """The same kernel (same plan: asserted) on more rows, on more columns and with padded leading dimensions gives the same bits
    where the problems overlap.  256 more rows / columns (128 for the 128 x 128 kernels): whole tiles, so every tile of the smaller
    problem keeps its shape.  A ring weight gradient changes its k-slices with the tile count, so its split is pinned by the
    workspace: two slabs each."""
    step = 256 if c.family in ("ring", "wgrad") else 128
    M2, N2 = c.M + step, c.N + step
    o = R.operands(M2, N2, c.K, c.in_dt, "scaled", DEV)
    ws = (lambda M, N: 2 * M * N * 4) if c.family == "wgrad" else (lambda M, N: None)
    ref = launch(c, o, ws=ws(c.M, c.N))
    plan = _plan(c, c.M, c.N, c.pc, ws(c.M, c.N))
    grown = 0
    for M, N in ((M2, c.N), (c.M, N2)):
        if _plan(c, M, N, c.pc, ws(M, N)) != plan:
            # the only such case: 16-bit split-K behind the LDS-DMA kernel at 136 rows -- from 256 rows on the plan sends this K
            # to the ring weight-gradient kernel, another kernel with another summation order
            assert (c.family, M, bool(c.ws), c.in_dt != "fp32") == ("lds128", M2, True, True), (G.case_id(c), M, N)
            continue
        grown += 1
        big = launch(c, o, M=M, N=N, ws=ws(M, N))
        for name in ref:
            assert torch.equal(big[name][:c.M, :c.N], ref[name]), f"{G.case_id(c)} {name}: other bits inside a {M} x {N} problem"
    assert grown
    if c.family == "ring" or (c.family in ("generic", "lds128") and not c.ws):   # (split-K needs ldc == N: lda / ldb only)
        epc = 4 if c.in_dt == "fp32" else 8
        for pads in ((epc, 0, 0), (0, epc, 0), (0, 0, 8), (0, 0, 4), (0, 0, 0)):
            if pads == (c.pa, c.pb, c.pc):
                continue
            if _plan(c, c.M, c.N, pads[2]) != plan:
                continue
            pad = launch(c, o, pads=pads)
            for name in ref:
                assert torch.equal(pad[name], ref[name]), f"{G.case_id(c)} {name}: other bits with paddings {pads}"
    else:
        epc = 8
        for pads in ((epc, 0, 0), (0, epc, 0)):
            pad = launch(c, o, pads=pads, ws=ws(c.M, c.N))
            assert torch.equal(pad["C"], ref["C"]), f"{G.case_id(c)}: other bits with paddings {pads}"


@pytest.mark.parametrize("c", [c for c in G.CASES if c.split > 1 and c.epi == "store" and c.in_dt != "fp16"], ids=G.case_id)
def test_split_k_against_whole_k(c):
    """The same problem in one slice (a 64-byte workspace: no slab fits) and in the case's k-slices: both inside the bound, and
    the ACCUM form equals the STORE form + C_in within b_acc + 2^-24 |C_in| (the one extra rounding of the sum)."""
    o, acc, T = _reference(c.M, c.N, c.K, c.in_dt, "scaled")
    assert _plan(c, c.M, c.N, 0, 64)[4] == 1 and _plan(c, c.M, c.N)[4] == c.split
    outs = {}
    for name, ws in (("whole", 64), ("split", None)):
        for epi in ("store", "accum"):
            outs[name, epi] = launch(c, o, ws=ws, epi=epi)
            judge(c, o, acc, T, outs[name, epi], f"{G.case_id(c)} {name}-K {epi}", epi=epi)
    base = o["base"].double()
    slack = R.b_acc(T, c.K) + 2.0 ** -24 * base.abs()
    for name in ("whole", "split"):
        diff = (outs[name, "accum"]["C"].double() - (outs[name, "store"]["C"].double() + base)).abs()
        assert bool((diff <= slack).all()), f"{G.case_id(c)} {name}-K: ACCUM differs from STORE + C_in by {(diff / slack).max().item():.3f} of the slack"


def test_refusals():
    """Every documented refusal returns its status, and C keeps its fill."""
    L = _lib()
    EAL, EINV = L.PM_EALIGN, L.PM_EINVAL
    o = R.operands(1031, 264, 64, "bf16", "uniform", DEV)
    c = G.Case("lds128", 0, "nt", "bf16", "bf16", "store", 136, 136, 64, 0, 0, 0, True, 0, 0, 1, 0, (128, 128), 0)
    launch(c, o)                                                         # (the base call is accepted)
    launch(c._replace(N=134), o, status=EAL, what="N & 3")
    launch(c, o, pads=(4, 0, 0), status=EAL, what="lda not a chunk multiple")
    launch(c, o, pads=(0, 4, 0), status=EAL, what="ldb not a chunk multiple")
    launch(c, o, pads=(0, 0, 2), status=EAL, what="ldc & 3")
    launch(c._replace(c_dt="fp16"), o, status=EINV, what="an fp16 C of bf16 operands")
    launch(c._replace(epi="resid"), o, status=EINV, what="RESIDUAL into a 16-bit C")
    launch(c._replace(epi="accum"), o, status=EINV, what="ACCUM into a 16-bit C")
    ring = c._replace(family="ring", variant=9, cfg=9, layout="nn", M=1031, N=264)
    launch(ring, o, status=EINV, what="ring cfg 9 with a k-major W")
    launch(ring._replace(variant=24, cfg=24), o)                         # (cfg 24 is built for it)
    # pointers: a misaligned A / B / C, and DGELU without its saved pre-activation
    DT, EPI = _codes()
    A, B = o["A"][:136].contiguous(), o["B"][:136].contiguous()
    Cbuf = torch.full((136 * 136 + 8,), FILL, dtype=torch.bfloat16, device=DEV)
    args = lambda a, b, cc, epi, aux: (a, 64, 0, b, 64, 0, DT["bf16"], None, cc, 136, DT["bf16"], EPI[epi], aux, None, 136, 136, 64,
                                       None, 0, None, _stream())
    lib = L.load()
    Abuf, Bbuf = torch.zeros(A.numel() + 8, dtype=A.dtype, device=DEV), torch.zeros(B.numel() + 8, dtype=B.dtype, device=DEV)
    assert lib.pm_gemm_ex(*args(Abuf.data_ptr() + 2, B.data_ptr(), Cbuf.data_ptr(), "store", None)) == EAL
    assert lib.pm_gemm_ex(*args(A.data_ptr(), Bbuf.data_ptr() + 2, Cbuf.data_ptr(), "store", None)) == EAL
    assert lib.pm_gemm_ex(*args(A.data_ptr(), B.data_ptr(), Cbuf.data_ptr() + 2, "store", None)) == EAL
    assert lib.pm_gemm_ex(*args(A.data_ptr(), B.data_ptr(), Cbuf.data_ptr(), "dgelu", None)) == EINV
    torch.cuda.synchronize()
    assert bool((Cbuf == FILL).all()), "a refused call wrote C"
