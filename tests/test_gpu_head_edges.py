"""pm_vit_head_fwd / pm_vit_head_bwd over a covering set of (B, N, D, pool, n_class, bias, head, regime) (tests/rowops_cases.py HEAD
says which combination reaches which branch), against the float64 reference and the element-wise bounds of tests/rowops_ref.py
(tests/test_rowops_ref_cpu.py holds them to f32 emulations): mean, rstd, feat, xhat_mean, logits; dx and dx_act in the three types
with their exact zero rows; dW, dbias, dgamma, dbeta added into prior contents at n 2^-24 T.  The backward is fed the float64
statistics rounded to f32, and chained once to the kernel's own forward at the norm-wise bounds of tests/test_gpu_ops.py.  Outputs
lie NaN-filled between guards.  Each test prints its largest err / bound per output (`pytest -s`)."""
import functools

import pytest
import torch

import rowops_cases as C
import rowops_ref as R
from test_gpu_attention_edges import _guarded, _guards_hold
from test_gpu_token_path_edges import abi, code, status, untouched

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from ssl4polyp_amd import _lib
    _lib.load()


@functools.lru_cache(maxsize=None)
def _case(case):
    """Operands on the device, the float64 forward, and the operands of the backward made from it (rounded to f32)."""
    B, N, D, pool, nk, has_bias, head, regime = case
    x, gamma, beta, W, bias, dlogits, dfeat = (t.to(DEV) for t in C.head_inputs(B, N, D, nk, regime))
    c = dict(x=x, gamma=gamma, beta=beta, W=W if head else None, bias=bias if (head and has_bias) else None,
             dlogits=dlogits if head else None, dfeat=None if head else dfeat)
    c["fwd"] = fwd = R.head_fwd(x, pool, gamma, beta, c["W"], c["bias"])
    c["mean_in"], c["rstd_in"], c["feat_in"] = fwd["mean"].float().contiguous(), fwd["rstd"].float().contiguous(), fwd["feat"].float()
    c["xhm_in"] = fwd["xhat_mean"].float() if pool == 1 else None
    c["prior"] = {n: C.randn(*s, seed=50 + i).to(DEV) for i, (n, s) in enumerate((("dW", (nk, D)), ("dbias", (nk,)), ("dgamma", (D,)), ("dbeta", (D,))))}
    c["bwd"] = R.head_bwd(c["dlogits"], c["dfeat"], x, pool, gamma, c["W"], c["feat_in"] if head else None, c["xhm_in"], c["mean_in"],
                          c["rstd_in"], c["prior"])
    return c


def _report(r, what):
    for k, v in r.items():
        print(f"{what} {k}: err/bound {v:.3f}")
    for k, v in r.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of its bound"


def _forward(case, c, what):
    B, N, D, pool, nk, _, head, _ = case
    rows = B if pool == 0 else B * N
    bufs = {n: _guarded(s, f32) for n, s in (("feat", (B, D)), ("xhm", (B, D)), ("mean", (rows,)), ("rstd", (rows,)), ("logits", (B, nk)))}
    o = {n: v for n, (_, v) in bufs.items()}
    assert abi("pm_vit_head_fwd", c["x"], N, pool, c["gamma"], c["beta"], c["W"], c["bias"], o["feat"], o["xhm"] if pool else None, o["mean"],
               o["rstd"], o["logits"] if head else None, B, D, nk, R.LN_EPS) == 0
    torch.cuda.synchronize()
    for n, (buf, _) in bufs.items():
        _guards_hold(buf, f"{what} {n}")
    if pool == 0:
        assert untouched(bufs["xhm"][0])
    if not head:
        assert untouched(bufs["logits"][0])
    return o


@pytest.mark.parametrize("case", C.HEAD)
def test_forward(case):
    B, N, D, pool, nk, _, head, regime = case
    c, what = _case(case), f"head fwd {case}"
    o, ref = _forward(case, c, what), _case(case)["fwd"]
    mean, rstd = o["mean"], o["rstd"]
    want_mean, want_rstd, e_mean, e_rstd = ref["mean"], ref["rstd"], ref["e_mean"], ref["e_rstd"]
    if pool == 1:   # the cls row has no statistics: never written
        mean, rstd = mean.view(B, N), rstd.view(B, N)
        assert bool(torch.isnan(mean[:, 0]).all()) and bool(torch.isnan(rstd[:, 0]).all())
        mean, rstd, want_mean, want_rstd, e_mean, e_rstd = (t[:, 1:] for t in (mean, rstd, want_mean, want_rstd, e_mean, e_rstd))
    r = {"mean": R.ratio(mean, want_mean, e_mean), "rstd": R.ratio(rstd, want_rstd, e_rstd), "feat": R.ratio(o["feat"], ref["feat"], ref["e_feat"])}
    if pool == 1:
        r["xhat_mean"] = R.ratio(o["xhm"], ref["xhat_mean"], ref["e_xhat_mean"])
    if head:
        r["logits"] = R.ratio(o["logits"], ref["logits"], ref["e_logits"])
    _report(r, what)


def _backward(case, c, prec, what, mean, rstd, feat, xhm, want_dx=True, sums=("dW", "dbias", "dgamma", "dbeta")):
    B, N, D, pool, nk, _, head, _ = case
    xb, dx = _guarded((B, N, D), f32)
    ab, dxa = _guarded((B, N, D), R.DTYPES[prec])
    g = {}
    for n in ("dW", "dbias", "dgamma", "dbeta"):
        if n in sums and (head or n in ("dgamma", "dbeta")):
            g[n] = _guarded(c["prior"][n].shape, f32)
            g[n][1].copy_(c["prior"][n])
    p = lambda n: g[n][1] if n in g else None
    assert abi("pm_vit_head_bwd", c["dlogits"], c["dfeat"], c["x"], N, pool, c["gamma"], c["W"], feat if head else None, xhm, mean, rstd,
               dx if want_dx else None, dxa if want_dx else None, code(dxa.dtype), p("dW"), p("dbias"), p("dgamma"), p("dbeta"), B, D, nk) == 0
    torch.cuda.synchronize()
    for buf, n in [(xb, "dx"), (ab, "dx_act")] + [(g[n][0], n) for n in g]:
        _guards_hold(buf, f"{what} {n}")
    if not want_dx:
        assert untouched(xb) and untouched(ab)
    return dx, dxa, {n: v[1] for n, v in g.items()}


@pytest.mark.parametrize("prec", C.PRECS)
@pytest.mark.parametrize("case", C.HEAD)
def test_backward_on_reference_statistics(case, prec):
    B, N, D, pool, nk, _, head, _ = case
    c, what = _case(case), f"head bwd {case} {prec}"
    ref = c["bwd"]
    dx, dxa, sums = _backward(case, c, prec, what, c["mean_in"], c["rstd_in"], c["feat_in"], c["xhm_in"])
    r = {"dx": R.ratio(dx, ref["dx"], ref["e_dx"]), "dx_act": R.ratio(dxa, ref["dx"], R.store_bound(ref["e_dx"], ref["dx"], prec))}
    for n, got in sums.items():
        r[n] = R.ratio(got, ref[n], R.sum_bound(ref["n_" + n], ref["t_" + n]))
    _report(r, what)
    zero_rows = (slice(None), slice(1, None)) if pool == 0 else (slice(None), slice(0, 1))
    for t in (dx, dxa):   # rows that do not reach the feature: exact zeros
        assert bool((t[zero_rows] == 0).all())
    # frozen backbone (dx = NULL): the same parameter gradients, bit for bit
    _, _, frozen = _backward(case, c, prec, what + " frozen", c["mean_in"], c["rstd_in"], c["feat_in"], c["xhm_in"], want_dx=False)
    for n in sums:
        assert torch.equal(sums[n], frozen[n]), n


@pytest.mark.parametrize("case", [C.HEAD[4], C.HEAD[9]])
def test_backward_chained_to_own_forward(case):
    """The kernel's own mean / rstd / feat / xhat_mean into its backward (cls at D = 1024, pooled over 49 rows), at the norm-wise bounds of
    tests/test_gpu_ops.py: dx, dgamma, dbeta 2e-5, dW, dbias 1e-5, dx_act 8e-3 (bf16)."""
    B, N, D, pool, nk, _, head, _ = case
    c = _case(case)
    o = _forward(case, c, "chained fwd")
    dx, dxa, sums = _backward(case, c, "bf16", "chained", o["mean"], o["rstd"], o["feat"], o["xhm"] if pool else None)
    fwd = c["fwd"]
    ref = R.head_bwd(c["dlogits"], c["dfeat"], c["x"], pool, c["gamma"], c["W"], fwd["feat"], fwd.get("xhat_mean"), fwd["mean"], fwd["rstd"],
                     c["prior"])
    errs = {"dx": (R.rel(dx, ref["dx"]), 2e-5), "dx_act": (R.rel(dxa, ref["dx"]), 8e-3)}
    for n, got in sums.items():
        errs[n] = (R.rel(got - c["prior"][n], ref[n] - c["prior"][n].double()), 2e-5 if n in ("dgamma", "dbeta") else 1e-5)
    for n, (e, b) in errs.items():
        print(f"chained {case} {n}: {e:.3e} (bound {b:.1e})")
        assert e < b, n


@pytest.mark.parametrize("what", ["fwd D = 1028", "fwd n_class = 257", "fwd D % 4", "fwd pool", "fwd pool N = 1", "fwd gamma NULL",
                                  "bwd D = 1028", "bwd n_class = 257", "bwd no gradient source", "bwd dx_act without dx", "bwd dtype"])
def test_refusals(what):
    src = torch.zeros(8192, device=DEV)
    buf, dst = _guarded((8192,), f32)
    fwd = lambda N=2, pool=0, gamma=src, D=64, nk=2: abi("pm_vit_head_fwd", src, N, pool, gamma, src, src, src, dst, dst, dst, dst, dst, 2, D, nk, 1e-6)
    bwd = lambda D=64, nk=2, dl=src, dx=dst, dxa=None, dt=0: abi("pm_vit_head_bwd", dl, None, src, 2, 0, src, src, src, None, src, src, dx, dxa, dt,
                                                                   dst, dst, dst, dst, 2, D, nk)
    got, want = {
        "fwd D = 1028": lambda: (fwd(D=1028), "ESHAPE"), "fwd n_class = 257": lambda: (fwd(nk=257), "ESHAPE"), "fwd D % 4": lambda: (fwd(D=66), "ESHAPE"),
        "fwd pool": lambda: (fwd(pool=2), "EINVAL"), "fwd pool N = 1": lambda: (fwd(N=1, pool=1), "ESHAPE"), "fwd gamma NULL": lambda: (fwd(gamma=None), "EINVAL"),
        "bwd D = 1028": lambda: (bwd(D=1028), "ESHAPE"), "bwd n_class = 257": lambda: (bwd(nk=257), "ESHAPE"),
        "bwd no gradient source": lambda: (bwd(dl=None), "EINVAL"), "bwd dx_act without dx": lambda: (bwd(dx=None, dxa=dst), "EINVAL"),
        "bwd dtype": lambda: (bwd(dxa=dst, dt=5), "EINVAL"),
    }[what]()
    torch.cuda.synchronize()
    assert got == status(want), what
    assert untouched(buf)
