"""pm_layernorm_fwd at the edges of its row scheduling (tests/rowops_cases.py), against the float64 reference and the element-wise
bounds of tests/rowops_ref.py (derived from the kernel's rounding points, no safety factor; tests/test_rowops_ref_cpu.py): mean,
rstd and y of every slot count, ragged slot, row count with idle waves, row pitch, input regime and output type; outputs NaN-filled
between guards; rows compared with the same rows of a larger launch, runs with a second run.  Each test prints its largest
err / bound per output (`pytest -s`); docs/EXPERIMENT_LOG.md has the table."""
import functools

import pytest
import torch

import rowops_cases as C
import rowops_ref as R
from test_gpu_attention_edges import _guarded, _guards_hold

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


def _call(x, ldx, gamma, beta, y, mean, rstd, M, D, dtype_code=None, eps=R.LN_EPS):
    """pm_layernorm_fwd through the C ABI (engine.Kernels.layernorm_fwd fixes ldx = D); -> its status."""
    from ssl4polyp_amd import _lib
    from ssl4polyp_amd.engine import _ptr, _stream
    code = _lib.dtype_code(y.dtype) if dtype_code is None else dtype_code
    return _lib.load().pm_layernorm_fwd(_ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(y), code, _ptr(mean), _ptr(rstd), M, D, eps, _stream())


def _pitched(x, pitch):
    """x [M, D] as a view of a NaN-filled buffer with the pitch asked for: what lies between the rows must never be read."""
    M, D = x.shape
    if pitch == "D":
        return x.contiguous(), D
    if pitch == "D+4":   # columns 4 .. 4 + D of a [M, D + 4] buffer
        buf = torch.full((M, D + 4), float("nan"), device=DEV)
        view = buf[:, 4:]
    else:                # token 0 of [M, 5, D]: the cls rows of a batch
        buf = torch.full((M, 5, D), float("nan"), device=DEV)
        view = buf[:, 0]
    view.copy_(x)
    return view, C.ln_pitch(D, pitch)


def _run(x, ldx, gamma, beta, M, D, prec, what, rows=None):
    """-> y, mean, rstd of `rows` rows (default M), allocated for M, NaN-filled between guards."""
    yb, y = _guarded((M, D), R.DTYPES[prec])
    mb, mean = _guarded((M,), torch.float32)
    rb, rstd = _guarded((M,), torch.float32)
    assert _call(x, ldx, gamma, beta, y, mean, rstd, M if rows is None else rows, D) == 0
    torch.cuda.synchronize()
    for buf, name in ((yb, "y"), (mb, "mean"), (rb, "rstd")):
        _guards_hold(buf, f"{what} {name}")
    return y, mean, rstd


@functools.lru_cache(maxsize=None)
def _case(M, D, regime):
    x = C.rows(M, D, regime).to(DEV)
    gamma, beta = (t.to(DEV) for t in C.affine(D))
    return x, gamma, beta, R.ln_fwd(x, gamma, beta)


def _check(y, mean, rstd, ref, prec, what):
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all()), \
        what + ": an output element was not written"
    r = R.ln_ratios(mean, rstd, y, ref, prec)
    for name, v in r.items():
        print(f"{what} {name}: err/bound {v:.3f}")
    for name, v in r.items():
        assert v <= 1.0, f"{what}: {name} at {v:.3f} of its bound"


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("M,D,regime", C.LN_CASES)
def test_rows_slots_regimes_pitches(M, D, regime, prec):
    """Every case at the three row pitches: each within the bounds, all three the same bits, and a second run the same bits."""
    x, gamma, beta, ref = _case(M, D, regime)
    outs = []
    for pitch in C.LN_PITCH:
        xv, ldx = _pitched(x, pitch)
        what = f"ln_fwd M={M} D={D} {regime} ldx={pitch} {prec}"
        outs.append(_run(xv, ldx, gamma, beta, M, D, prec, what))
        _check(*outs[-1], ref, prec, what)
    outs.append(_run(x, D, gamma, beta, M, D, prec, "second run"))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("prec", C.PRECS)
def test_grid_stride_second_trip(prec):
    """M = 16389: the grid is capped at 4096 workgroups of four rows, the last five rows are a second trip."""
    M, D = C.LN_GRID
    x, gamma, beta, ref = _case(M, D, "random")
    y, mean, rstd = _run(x, D, gamma, beta, M, D, prec, "grid")
    _check(y, mean, rstd, ref, prec, f"ln_fwd M={M} D={D} {prec}")


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("D", [768, 1028])
def test_row_locality(D, prec):
    """A row's outputs depend neither on the wave that handled it nor on its neighbours: rows [0, 37) of an M = 1000 run are the
    M = 37 run, and a launch of 37 rows writes nothing past them."""
    x, gamma, beta, _ = _case(1000, D, "random")
    big = _run(x, D, gamma, beta, 1000, D, prec, "M=1000")
    small = _run(x, D, gamma, beta, 1000, D, prec, "M=37 of 1000", rows=37)
    for a, b in zip(big, small):
        assert torch.equal(a[:37], b[:37])
        assert bool(torch.isnan(b[37:].float()).all())


@pytest.mark.parametrize("what,kw,status", [
    ("D over 1280", dict(D=1284), "ESHAPE"), ("D not a multiple of 4", dict(D=66), "ESHAPE"), ("ldx not a multiple of 4", dict(ldx=70), "ESHAPE"),
    ("M = 0", dict(M=0), "ESHAPE"), ("x NULL", dict(null="x"), "EINVAL"), ("rstd NULL", dict(null="rstd"), "EINVAL"),
    ("unknown dtype", dict(code=7), "EINVAL")])
def test_refusals(what, kw, status):
    """Rejected before any launch: the exact status, and the NaN-filled outputs untouched."""
    from ssl4polyp_amd import _lib
    M, D = kw.get("M", 3), kw.get("D", 68)
    x, gamma, beta = torch.zeros(3, 1288, device=DEV), torch.ones(1288, device=DEV), torch.zeros(1288, device=DEV)
    yb, y = _guarded((3, 1288), torch.bfloat16)
    mb, mean = _guarded((3,), torch.float32)
    rb, rstd = _guarded((3,), torch.float32)
    args = dict(x=x, gamma=gamma, beta=beta, y=y, mean=mean, rstd=rstd)
    if "null" in kw:
        args[kw["null"]] = None
    got = _call(args["x"], kw.get("ldx", 1288), args["gamma"], args["beta"], args["y"], args["mean"], args["rstd"], M, D, dtype_code=kw.get("code", 1))
    torch.cuda.synchronize()
    assert got == getattr(_lib, "PM_" + status), what
    for t in (yb[256:-256], mb[256:-256], rb[256:-256]):
        assert bool(torch.isnan(t.float()).all()), what + ": an output was written"
