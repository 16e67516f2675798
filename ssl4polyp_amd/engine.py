"""Host-side execution engine: sequences the HIP kernels of one ViT / MAE training step.

This is the MI355X-native counterpart of the torch/timm op graph that the reference builds in
``MaskedAutoencoderViT.forward`` (src/ssl4polyp/models/mae/models_mae.py:150-220) and
``ViT_from_MAE.forward`` / ``VisionTransformer_from_Any.forward`` (src/ssl4polyp/models/models.py:117-140,
196-222) plus autograd's backward of it.  Instead of ~14 library launches per block with the [N,N]
attention scores, GELU and residual tensors round-tripping HBM, a block is 7 launches forward
(LN, qkv GEMM, fused attention, proj GEMM+residual, LN, fc1 GEMM+GELU, fc2 GEMM+residual) and the whole
forward/backward is ONE autograd node, so the engine owns every intermediate buffer, their dtypes
(bf16 activations, f32 residual stream and statistics) and the order in which gradients become ready
(which drives the RCCL bucket all-reduce, see parallel.py).

PyTorch is used for device memory (caching allocator), streams and autograd plumbing only; all
arithmetic is in libpolypmae.so.  No CPU / eager fallback exists.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import contextlib
import ctypes
import os

import torch

from . import _lib
from ._lib import EPI_ACCUM, EPI_DGELU, EPI_GELU, EPI_RESIDUAL, EPI_STORE, PM_BF16, PM_F16, PM_F32

LN_EPS = 1e-6  # models_mae.py:227, models.py:164: partial(nn.LayerNorm, eps=1e-6)

BLOCK_PARAM_NAMES = (
    "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
    "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """hipStream_t of torch's current stream.  Called once per launch (~450 times per step, forward + backward): the raw getters
    cost ~0.3 us, `torch.cuda.current_stream().cuda_stream` ~8 us (device-index resolution + a Stream object per call) --
    1.8 ms of a ViT-B step's 6 ms host enqueue time."""
    if _raw_stream is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _stream_key(stream: Optional["torch.cuda.Stream"] = None) -> Tuple[int, int]:
    """(device index, hipStream_t) of `stream`; by default of torch's current stream, the one a launch goes to."""
    if stream is not None:
        return stream.device.index, stream.cuda_stream
    if _raw_stream is not None:
        dev = _cur_device()
        return dev, _raw_stream(dev)
    st = torch.cuda.current_stream()
    return st.device.index, st.cuda_stream


class ScratchArena:
    """One byte buffer per key that only ever grows.  The engine keys it by stream: kernels on one stream run one after the other,
    and every launch that fills scratch is followed by the launch that reads it on the same stream inside the same C call, so one
    buffer per stream is always enough -- and two streams never share one.  Growing a buffer (first step of a new shape) drains
    the device first: a launch still in flight may be using the old one.  (Not while a graph is being captured: nothing executes
    then, and a capture runs on a stream of its own, so its first step sizes that stream's buffer.)"""

    FLOOR = 1 << 16

    def __init__(self):
        self.bufs: Dict[object, torch.Tensor] = {}
        self.generation = 0   # bumped whenever a buffer is created or replaced: whoever keeps a pointer compares it

    def get(self, key, nbytes: int, device) -> torch.Tensor:
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None and buf.is_cuda and not torch.cuda.is_current_stream_capturing():
                torch.cuda.synchronize(device)
            buf = self.bufs[key] = torch.empty(max(nbytes, self.FLOOR), dtype=torch.uint8, device=device)
            self.generation += 1
        return buf


_STREAMS: Dict[Tuple[int, str], "torch.cuda.Stream"] = {}
# The second weight-gradient stream (busy in the backward only) IS the second forward chain's stream (busy in the forward only):
# two engine streams + the main stream = three busy streams, each on a hardware queue of its own under the runtime's default of four,
# and one queue left for RCCL in a data-parallel rank (scratch/archive_r3/r3_exp23.sh)


def _shared_stream(device, role: str):
    """The process-wide side stream of this role ("aux0", "side", ...) on `device`, created on first use."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), role)
    st = _STREAMS.get(key)
    if st is None:
        st = _STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


def reserve_streams(device) -> None:
    """Create the engine's side streams on `device` and put one tiny launch on each, NOW.  The HIP runtime binds a stream to one
    of its few hardware queues (GPU_MAX_HW_QUEUES, 4) when the stream is first used -- a new queue while there are fewer than
    that, the least-loaded one afterwards: called before anything else uses streams -- in particular before torch.distributed /
    RCCL initialise, which use half a dozen of their own -- the main stream and the two side streams each get a queue to
    themselves and the fourth is left for RCCL.  Called late, two of them can land on one queue and run one after the other
    (measured with RCCL initialised first: the second forward chain behind the main stream, cls step 15.0 instead of 10.6 ms)."""
    dev = torch.device(device)
    torch.zeros(1, device=dev)  # (the main stream first)
    for role in ("aux0", "side"):
        with torch.cuda.stream(_shared_stream(dev, role)):
            torch.zeros(1, device=dev)
    torch.cuda.synchronize(dev)


# precision mode -> (activation / matrix-shadow dtype, its C-ABI code).  bf16: v_mfma_f32_32x32x16_bf16, no loss scaling.
# fp16: the reference's own AMP arithmetic (torch.cuda.amp.autocast = fp16 matmuls with f32 accumulation + GradScaler:
# train_classification.py:4527-4546, engine_pretrain.py:52-72) on v_mfma_f32_32x32x16_f16 -- same rate, 11 significant bits per
# operand instead of 8 (logits 4x closer to the fp32 path, gradients 7x: profiles/r4_rounding_fp16_*.json); the backward runs on
# fp16 operands too, so the loss must be scaled (optim.LossScaler, or torch's GradScaler).  fp32: exact-f32 MFMA, 1/16 of the rate.
PRECISIONS = {"bf16": (torch.bfloat16, PM_BF16), "fp16": (torch.float16, PM_F16), "fp32": (torch.float32, PM_F32)}


class Kernels:
    """Thin typed wrappers: torch tensors in, C-ABI calls out (include/polypmae.h)."""

    # The switches: what the tests and bench.py flip per object, and a whole-process A/B run by the environment variable.
    SPLIT_FORWARD = int(os.environ.get("PM_SPLIT_FWD", "2"))     # The forward runs as this many sub-batches on concurrent streams (1 = off).
    # Workgroups a split-K weight gradient takes beside the dgrad chain on the main stream (pm_gemm_opts.max_blocks; 128 best of 96..256).
    WGRAD_BLOCKS = int(os.environ.get("PM_WGRAD_BLOCKS", "128"))
    # A whole-K block's weight gradients go out as (fc2, fc1) behind dfc2 and (proj, qkv) behind the attention backward, on two side streams.
    TWO_GROUPS = os.environ.get("PM_TWO_GROUPS", "1") == "1"
    TIME_BLOCK_EVENTS = False                                    # The fork / done events of pm_vit_block_bwd carry timestamps (bench.py times its weight gradients by them).
    gemm_variant = int(os.environ.get("PM_GEMM_VARIANT", "0"))   # pm_gemm_opts.variant of every GEMM: 0 = the dispatcher's heuristics.
    BLOCK_CALLS = os.environ.get("PM_BLOCK_CALLS", "1") != "0"   # A block is ONE C call (pm_vit_block_fwd / pm_vit_block_bwd) instead of a call per kernel.
    GROUP_BLOCKS = int(os.environ.get("PM_GROUP_BLOCKS", "0"))   # CUs a grouped weight-gradient launch may take (0 = one workgroup per tile).
    GROUP_BLOCKS_SLICED = int(os.environ.get("PM_GROUP_BLOCKS_SLICED", "0"))  # The same for a k-sliced group (0 = one workgroup per tile and slice).
    # A block's weight gradients are one grouped launch from this many 256x256 tiles on, and below it when the library k-slices them (0 = always).
    GROUP_MIN_TILES = int(os.environ.get("PM_GROUP_MIN_TILES", "64"))
    # The lowest trainable blocks of a stack that ends the pass, this many, issue their four weight gradients one by one (no dgrad chain runs beside them).
    UNGROUP_TAIL = int(os.environ.get("PM_UNGROUP_TAIL", "1"))
    SPARSE_TOP = os.environ.get("PM_SPARSE_TOP", "1") != "0"     # The classifier's top block runs on its cls rows behind the attention (backward too).

    def __init__(self, precision: str, eps: float = LN_EPS):
        self.eps = float(eps)
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'bf16', 'fp16' or 'fp32'")
        self.lib = _lib.load()
        self.precision = precision
        self.act_dtype, self.act = PRECISIONS[precision]
        self._need_cache: Dict[tuple, object] = {}      # what the library answered per shape: workspace bytes, grouping plans
        self._opts_cache: Optional[tuple] = None        # ((WGRAD_BLOCKS, gemm_variant), weight-gradient pm_gemm_opts, the others')
        self._side = self._side2 = None                 # the two weight-gradient streams, once a backward has asked for them
        self._arena = ScratchArena()                    # split-K slabs and partial rows: one buffer per (device, stream)

    # -- helpers ------------------------------------------------------------------------------
    def layernorm_fwd(self, x, gamma, beta, y, mean, rstd, M, D):
        _lib.check(self.lib.pm_layernorm_fwd(_ptr(x), D, _ptr(gamma), _ptr(beta), _ptr(y), _lib.dtype_code(y.dtype),
                                             _ptr(mean), _ptr(rstd), M, D, self.eps, _stream()), "pm_layernorm_fwd")

    def layernorm_bwd(self, dy, x, gamma, mean, rstd, dres, dx, dx_act, dgamma, dbeta, dcolsum, M, D):
        need = self._ln_bwd_bytes(M, D)
        ws = self._scratch(need, x.device)
        _lib.check(self.lib.pm_layernorm_bwd(_ptr(dy), _lib.dtype_code(dy.dtype), _ptr(x), D, _ptr(gamma), _ptr(mean),
                                             _ptr(rstd), _ptr(dres), D, _ptr(dx), D, _ptr(dx_act), self.act,
                                             _ptr(dgamma), _ptr(dbeta), _ptr(dcolsum), M, D, _ptr(ws), need, _stream()),
                   "pm_layernorm_bwd")

    # -- scratch: sized by the library's own queries (pm_gemm_workspace_bytes / pm_workspace_bytes, cached per shape), taken
    #    from the arena of the stream the launch goes to; the library is told the size it asked for, not the arena's
    def _need(self, key, query) -> int:
        n = self._need_cache.get(key)
        if n is None:
            n = self._need_cache[key] = int(query())
        return n

    def _ln_bwd_bytes(self, M: int, D: int) -> int:
        return self._need(("ln", M, D), lambda: self.lib.pm_workspace_bytes(_lib.WS_LAYERNORM_BWD, M, D))

    def _scratch(self, nbytes: int, device, stream: Optional["torch.cuda.Stream"] = None) -> torch.Tensor:
        """At least `nbytes` of the scratch of `stream` (default: the current one, where the launch goes)."""
        return self._arena.get(_stream_key(stream), nbytes, device)

    @staticmethod
    def _shape_items(dims):
        """The pm_wgrad_item array of (n_out, n_in[, has dbias]) gradients for the library's plan and workspace queries: shapes
        only, every pointer a stand-in that passes the alignment checks."""
        arr = (_lib.WgradItem * len(dims))()
        for j, (o, i, *bias) in enumerate(dims):
            arr[j] = _lib.WgradItem(64, o, 64, i, 64, i, o, i, 0, 64 if bias and bias[0] else None)
        return arr

    # The side streams are shared by every Kernels object of the process (one set per device): the HIP runtime multiplexes
    # streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and two streams on one queue run their
    # kernels one after the other.  A stream set per model put the third model's weight-gradient stream onto the main
    # stream's queue (bench.py builds several models in one process: the MAE step lost 11 %).
    def aux_stream(self, device, j: int = 0):
        return _shared_stream(device, f"aux{j}")

    def side_stream(self, device):
        st = self._side
        if st is None or st.device != device:
            st = self._side = _shared_stream(device, "side")
        return st

    def side_stream2(self, device):
        """The second weight-gradient stream (busy in the backward only) IS the second forward chain's (busy in the forward only)."""
        st = self._side2
        if st is None or st.device != device:
            st = self._side2 = _shared_stream(device, "aux0")
        return st

    def _opts(self, wgrad: bool):
        o = self._opts_cache
        if o is None or o[0] != (self.WGRAD_BLOCKS, self.gemm_variant):
            key = (self.WGRAD_BLOCKS, self.gemm_variant)
            o = self._opts_cache = (key, _lib.GemmOpts(self.WGRAD_BLOCKS, self.gemm_variant), _lib.GemmOpts(0, self.gemm_variant))
        return o[1] if wgrad else o[2]

    def gemm(self, A, lda, a_kmajor, B, ldb, b_kmajor, bias, C, ldc, epilogue, M, N, K, aux=None, resid=None):
        in_dtype = _lib.dtype_code(A.dtype)
        if _lib.dtype_code(B.dtype) != in_dtype:
            raise _lib.PolypMaeError("pm_gemm: operand dtypes differ")
        wgrad = bool(a_kmajor and b_kmajor)
        opts = self._opts(wgrad)
        ws, need = None, 0
        if wgrad:
            # a weight gradient always gets a workspace pointer, with 0 bytes where no split fits: that the caller HAS one is what
            # sends a long reduction to the weight-gradient ring kernel (plan_gemm: `splittable`), whatever the split count
            need = self._need(("gemm", in_dtype, M, N, K, opts.max_blocks, opts.variant),
                              lambda: self.lib.pm_gemm_workspace_bytes(1, 1, in_dtype, M, N, K, ctypes.byref(opts)))
            ws = self._scratch(need, A.device)
        _lib.check(self.lib.pm_gemm_ex(_ptr(A), lda, int(a_kmajor), _ptr(B), ldb, int(b_kmajor), in_dtype, _ptr(bias),
                                       _ptr(C), ldc, _lib.dtype_code(C.dtype), epilogue, _ptr(aux), _ptr(resid), M, N, K,
                                       _ptr(ws), need, ctypes.byref(opts), _stream()), "pm_gemm")

    def linear_fwd(self, x, W, bias, out, M, N, K, epilogue=EPI_STORE, aux=None, resid=None):
        """out[M,N] = x[M,K] @ W[N,K]^T + bias  (nn.Linear forward)."""
        self.gemm(x, K, 0, W, K, 0, bias, out, N, epilogue, M, N, K, aux=aux, resid=resid)

    def linear_dgrad(self, dy, W, dx, M, N_out, K_in, epilogue=EPI_STORE, aux=None):
        """dx[M,K_in] = dy[M,N_out] @ W[N_out,K_in]  (W read as stored: k-major B operand)."""
        self.gemm(dy, N_out, 0, W, K_in, 1, None, dx, K_in, epilogue, M, K_in, N_out, aux=aux)

    def wgrad_group(self, items, K, whole_k: bool = False) -> bool:
        """items: [(dy [K, n_out], x [K, n_in], dW f32 [n_out, n_in], accumulate[, dbias f32 [n_out] (+=)])].  One launch for all
        (pm_wgrad_group; a group of few tiles and long K is cut into k-slices: slabs in a scratch buffer sized by
        pm_wgrad_group_workspace_bytes, one reduce launch); False when the shapes do not fit the grouped kernel (the caller
        then uses linear_wgrad).  whole_k: PM_GROUP_WHOLE_K -- never slice (the second launch of a two-launch block)."""
        n = len(items)
        arr = (_lib.WgradItem * n)()
        for j, (dy, x, dW, acc, *rest) in enumerate(items):
            n_out, n_in = dW.shape
            arr[j] = _lib.WgradItem(_ptr(dy), n_out, _ptr(x), n_in, _ptr(dW), n_in, n_out, n_in, int(bool(acc)),
                                    _ptr(rest[0]) if rest and rest[0] is not None else None)
        dt = _lib.dtype_code(items[0][0].dtype)
        key = ("group", K, dt, tuple((tuple(it[2].shape), len(it) > 4 and it[4] is not None) for it in items))
        need = 0 if whole_k else self._need(key, lambda: self.lib.pm_wgrad_group_workspace_bytes(arr, n, K, dt))
        ws = self._scratch(need, items[0][0].device) if need else None
        blocks = _lib.PM_GROUP_WHOLE_K if whole_k else (self.GROUP_BLOCKS_SLICED if need else self.GROUP_BLOCKS)
        st = self.lib.pm_wgrad_group(arr, n, K, dt, blocks, _ptr(ws), need, _stream())
        if st == _lib.PM_ESHAPE:
            return False
        _lib.check(st, "pm_wgrad_group")
        return True

    def can_group_wgrad(self, K: int, dims) -> bool:
        """Would pm_wgrad_group take these (n_out, n_in) gradients over K tokens, and does the engine want it to?  The
        admission rules are the LIBRARY's (pm_wgrad_group_plan: bf16, whole 32-token k-steps, K >= 2048, tiles of at least
        256 x 128, 16-byte alignment) -- asked, not restated here; the policy on top is the engine's."""
        key = ("can_group", K, self.act, tuple(dims), self.GROUP_MIN_TILES)
        cache = self._need_cache
        hit = cache.get(key)
        if hit is not None:
            return hit
        tiles, slices = ctypes.c_int(0), ctypes.c_int(0)
        st = self.lib.pm_wgrad_group_plan(self._shape_items(dims), len(dims), K, self.act, None, ctypes.byref(tiles), ctypes.byref(slices))
        # >= 64 tiles of 256x256 (ViT-B block: 108): one full-K tile per workgroup.  Fewer (the 512-wide MAE decoder block:
        # 48) group as well when the library's plan cuts every tile into k-slices (48 tiles x 4 slices of >= 128 k-steps);
        # otherwise the gradients keep the per-GEMM split-K path (PM_GROUP_MIN_TILES=0 forces grouping: whole-K 256x128 tiles).
        ok = st == 0 and (tiles.value >= self.GROUP_MIN_TILES or slices.value > 1)
        cache[key] = ok
        return ok

    def two_launch_group(self, K: int, dims) -> bool:
        """May a grouped block (dims = fc2, fc1, proj, qkv) go out as two launches -- (fc2, fc1) and (proj, qkv) -- on two side
        streams (pm_block_bwd_desc.two_groups)?  Yes when the first pair alone is a whole-K group by the library's plan (no
        slabs: the two launches must not share a workspace); the second pair then runs whole-K too (PM_GROUP_WHOLE_K)."""
        if not self.TWO_GROUPS:
            return False
        key = ("two_launch", K, self.act, tuple(dims))
        cache = self._need_cache
        hit = cache.get(key)
        if hit is None:
            ok = True
            for first, part in ((True, dims[:2]), (False, dims[2:])):
                slices = ctypes.c_int(0)
                st = self.lib.pm_wgrad_group_plan(self._shape_items(part), 2, K, self.act, None, None, ctypes.byref(slices))
                ok = ok and st == 0 and (slices.value == 1 or not first)
            hit = cache[key] = ok
        return hit

    def linear_wgrad(self, dy, x, dW, M, N_out, K_in, accumulate):
        """dW[N_out,K_in] (+)= dy[M,N_out]^T @ x[M,K_in]  (both operands k-major, f32 output; split-K slabs in the current
        stream's scratch)."""
        self.gemm(dy, N_out, 1, x, K_in, 1, None, dW, K_in, EPI_ACCUM if accumulate else EPI_STORE, N_out, K_in, M)

    def colsum(self, x, out, M, N):
        need = self._need(("cs", M, N), lambda: self.lib.pm_workspace_bytes(_lib.WS_COLSUM, M, N))
        ws = self._scratch(need, x.device)
        _lib.check(self.lib.pm_colsum_ws(_ptr(x), N, _lib.dtype_code(x.dtype), _ptr(out), M, N, _ptr(ws), need, _stream()),
                   "pm_colsum")

    # -- stochastic depth (pm_droppath.hip): per-sample scales of a residual branch, scale f32 [M / N]
    def drop_path_add(self, x, y, out, scale, M, N, D):
        """out[r] = x[r] + scale[r // N] * y[r] over M rows of D f32 (out may be y)."""
        _lib.check(self.lib.pm_drop_path_add(_ptr(x), _ptr(y), _ptr(out), _ptr(scale), M, N, D, _stream()), "pm_drop_path_add")

    def drop_path_scale_cast(self, dy, scale, dy_act, colsum, M, N, D):
        """dy_act[r] = act(scale[r // N] * dy[r]); colsum (f32 [D], None: not wanted) += the column sums of the scaled rows."""
        need = self._need(("droppath", M, D), lambda: _lib.workspace_bytes("pm_drop_path_workspace", M, D)) if colsum is not None else 0
        ws = self._scratch(need, dy.device) if need else None
        _lib.check(self.lib.pm_drop_path_scale_cast(_ptr(dy), _ptr(scale), _ptr(dy_act), _lib.dtype_code(dy_act.dtype), _ptr(colsum),
                                                    M, N, D, _ptr(ws), need, _stream()), "pm_drop_path_scale_cast")

    def attention_fwd(self, qkv, out, lse, B, N, H, dh):
        _lib.check(self.lib.pm_attention_fwd(_ptr(qkv), _ptr(out), _ptr(lse), B, N, H, dh, self.act, _stream()),
                   "pm_attention_fwd")

    def attention_bwd(self, qkv, out, dout, lse, delta, dqkv, B, N, H, dh):
        _lib.check(self.lib.pm_attention_bwd(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(delta), _ptr(dqkv), B, N,
                                             H, dh, self.act, _stream()), "pm_attention_bwd")

    def mae_unshuffle_bwd(self, dx, ids_shuffle, demb, dmask_token, B, L, keep, D):
        """Backward of pm_mae_unshuffle: dx f32 [B (L + 1), D] -> demb act [B (keep + 1), D], the masked rows summed into dmask_token
        (f32 [D], += ; None: frozen) in a fixed order through partial rows."""
        need = self._need(("unshuf", D), lambda: self.lib.pm_workspace_bytes(_lib.WS_UNSHUFFLE_BWD, 1, D))
        ws = self._scratch(need, dx.device)
        _lib.check(self.lib.pm_mae_unshuffle_bwd(_ptr(dx), _ptr(ids_shuffle), _ptr(demb), self.act, _ptr(dmask_token), B, L, keep, D,
                                                 _ptr(ws), need, _stream()), "pm_mae_unshuffle_bwd")

    def gather_rows(self, src: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dst[r] = src[idx[r]] for a 2-D (or 1-D) contiguous src; idx int32 on the device; out: a contiguous [R, width] destination."""
        rows = src if src.ndim == 2 else src.view(-1, 1)
        dst = out if out is not None else torch.empty(idx.numel(), rows.shape[1], dtype=src.dtype, device=src.device)
        rb = rows.shape[1] * src.element_size()
        _lib.check(self.lib.pm_gather_rows(_ptr(rows), rb, _ptr(idx), _ptr(dst), idx.numel(), rb, _stream()), "pm_gather_rows")
        return dst if src.ndim == 2 else dst.view(-1)

    def scatter_rows_zero(self, src: torch.Tensor, inv: torch.Tensor, dst: torch.Tensor) -> None:
        """dst[m] = src[inv[m]] where inv[m] >= 0, zeros elsewhere (every row of dst is written)."""
        _lib.check(self.lib.pm_scatter_rows_zero(_ptr(src), _ptr(inv), _ptr(dst), dst.shape[0], dst.shape[1] * dst.element_size(),
                                                 _stream()), "pm_scatter_rows_zero")

    def cast(self, src, dst):
        _lib.check(self.lib.pm_cast(_ptr(src), _ptr(dst), _lib.dtype_code(dst.dtype), src.numel(), _stream()), "pm_cast")

    # A Linear whose reduction dimension is not a multiple of the GEMM k-step (patch 14: 3 * 14 * 14 = 588) runs in a layout
    # padded with zeros to the next multiple of 64: operands by pad_cast, the valid part of a gradient back by unpad_add.
    @staticmethod
    def padded_k(K: int) -> int:
        return K if K % 64 == 0 else (K + 63) // 64 * 64

    def pad_cast(self, src: torch.Tensor, rows_pad: int, cols_pad: int) -> torch.Tensor:
        """f32 [rows, cols] -> act [rows_pad, cols_pad], zeros outside the source."""
        rows, cols = src.shape
        dst = torch.empty(rows_pad, cols_pad, dtype=self.act_dtype, device=src.device)
        _lib.check(self.lib.pm_pad_cast(_ptr(src), cols, _ptr(dst), cols_pad, self.act, rows, cols, rows_pad, cols_pad, _stream()),
                   "pm_pad_cast")
        return dst

    def unpad_add(self, src: torch.Tensor, dst: torch.Tensor, accumulate: bool) -> None:
        """dst f32 [rows, cols] (+)= src f32 [>= rows, >= cols][:rows, :cols]."""
        rows, cols = dst.shape
        _lib.check(self.lib.pm_unpad_add(_ptr(src), src.shape[1], _ptr(dst), cols, rows, cols, 1 if accumulate else 0, _stream()),
                   "pm_unpad_add")


@dataclass
class StackGeom:
    """Geometry of one stack of pre-LN transformer blocks (timm Block)."""
    dim: int
    heads: int
    depth: int
    hidden: int

    @property
    def dh(self) -> int:
        return self.dim // self.heads


class BlockWorkspace:
    """Saved-for-backward activations of one block at (B, N).  Everything the backward needs, nothing else."""

    def __init__(self, g: StackGeom, B: int, N: int, act_dtype, dev):
        M, D, Hd = B * N, g.dim, g.hidden
        f32 = torch.float32
        e = lambda *s, dt=act_dtype: torch.empty(*s, dtype=dt, device=dev)
        self.mean1, self.rstd1 = e(M, dt=f32), e(M, dt=f32)
        self.ln1 = e(M, D)
        self.qkv = e(M, 3 * D)
        self.lse = e(B * g.heads * N, dt=f32)
        self.attn = e(M, D)
        self.x_mid = e(M, D, dt=f32)
        self.mean2, self.rstd2 = e(M, dt=f32), e(M, dt=f32)
        self.ln2 = e(M, D)
        self.h_pre = e(M, Hd)
        self.h_act = e(M, Hd)
        self.x_out = e(M, D, dt=f32)


class StackWorkspace:
    """Per-(B,N) buffers of a whole block stack: per-block saves + shared backward temporaries."""

    def __init__(self, g: StackGeom, B: int, N: int, act_dtype, dev, training: bool):
        self.B, self.N, self.M = B, N, B * N
        M, D, Hd = self.M, g.dim, g.hidden
        f32 = torch.float32
        nblk = g.depth if training else min(g.depth, 2)
        self.blocks = [BlockWorkspace(g, B, N, act_dtype, dev) for _ in range(nblk)]
        self.training = training
        if training:
            e = lambda *s, dt=act_dtype: torch.empty(*s, dtype=dt, device=dev)
            # The weight-gradient GEMMs of block i run on a side stream and may still be in flight while the main
            # stream is one block further down (see BlockStack.backward): what they read is double-buffered by block
            # parity (d_hidden, d_qkv) or rotates through five buffers (act copies of the residual gradient: block i
            # uses slots p, p+1, p+2, block i-1 slots p+2, p+3, p+4).
            self.d_hidden = [e(M, Hd), e(M, Hd)]
            self.d_qkv = [e(M, 3 * D), e(M, 3 * D)]
            self.d_ln = e(M, D)
            self.d_attn = e(M, D)
            self.delta = e(B * g.heads * N, dt=f32)
            self.dx = [e(M, D, dt=f32), e(M, D, dt=f32)]
            self.dx_act = [e(M, D) for _ in range(5)]
        # what BlockStack keeps here between calls
        self._fwd_descs: Dict[tuple, tuple] = {}   # (block, sample range) -> (key, pm_block_fwd_desc)
        self._bwd_descs: Dict[int, tuple] = {}     # block -> (key, pm_block_bwd_desc, done events, objects kept alive)
        self._top_c: Optional[dict] = None         # the cls-row top block's compact buffers (BlockStack.top_compact)
        self._deferred_join: list = []             # events a backward(defer_join=True) left for join_deferred
        self.cls_top = False                       # the last forward ran its top block on the cls rows: its result is [B, D]
        self._drop_zero: Optional[torch.Tensor] = None  # f32 [M, D] zeros: the "residual" of a branch GEMM under stochastic depth

    def block(self, i: int) -> BlockWorkspace:
        return self.blocks[i if self.training else i % len(self.blocks)]


_MLP_HALF_BUFFERS = ("x", "attn", "x_mid", "ln2", "mean2", "rstd2", "h_pre", "h_act", "x_out")  # BlockStack._mlp_half, in its order


class BlockStack:
    """Runs `depth` transformer blocks forward / backward over an f32 residual stream."""

    def __init__(self, k: Kernels, g: StackGeom):
        self.k, self.g = k, g

    @staticmethod
    def fork(src, dst):
        """Everything enqueued on `src` so far happens before whatever `dst` is given next (a fresh event per fork: an event still
        waited for by an overlapped optimizer update must not be re-recorded)."""
        ev = torch.cuda.Event()
        ev.record(src)
        dst.wait_event(ev)

    def forward(self, ws: StackWorkspace, x_in: torch.Tensor, W: Sequence[Dict[str, torch.Tensor]],
                before_block: Optional[Callable[[int], None]] = None, keep_from: int = 0, cls_top: bool = False,
                drop_scales: Optional[torch.Tensor] = None, drop_blocks: Optional[Sequence[bool]] = None) -> torch.Tensor:
        """x_in f32 [M, D]; W[i] maps BLOCK_PARAM_NAMES -> tensors (matrices act-typed, vectors f32).
        before_block(i) runs before block i's first kernel (gate on a pending optimizer update of its weights).
        keep_from: no backward will run through blocks below this index (frozen blocks under a frozen front: finetune.py:49-91), so
        fc1's GELU epilogue does not store their pre-activations (38.7 MB per launch at ViT-B, bs = 64); a forward-only workspace
        (evaluation, linear probe) keeps none.
        cls_top: the caller reads row 0 of every sample of the result only (out_token "cls", models.py:134-136).  Behind its attention,
        the TOP block is then per-token work whose other rows nobody reads: proj + residual, LayerNorm2, fc1 + GELU, fc2 + residual run
        on the B cls rows (gathered behind the attention), and the result comes back as [B, D] (= [B, 1, D] for the head kernels).
        Whether the stack took that path (it needs N > 1 and a block to run) is left in `ws.cls_top`, where the backward and the
        caller read it; a training workspace takes it at a batch that is a multiple of 8 only, and is refused here otherwise.
        drop_scales: stochastic depth -- f32 [depth, 2, B] on the device, the scale of sample b in the attention (0) / MLP (1) branch
        of block i: x = x + s[b] * branch.  None: every launch below is what it was without the argument.  With a table, the blocks
        named by drop_blocks (default: all) run kernel by kernel: proj and fc2 write the biased branch in f32 (EPI_RESIDUAL against
        zeros, the plan these GEMMs have anyway) and pm_drop_path_add makes x_mid / x_out in place; the other blocks take today's
        launches (their rows of the table must be 1).  The cls-row top block is off with a table.  The backward must get the same two
        arguments."""
        k, g = self.k, self.g
        if not ws.training:
            keep_from = g.depth
        B, N, D = ws.B, ws.N, g.dim
        drop = self._drop_plan(ws, drop_scales, drop_blocks)
        if drop is not None:
            cls_top = False
            if any(drop) and ws._drop_zero is None:  # (filled on this stream, before the fork below)
                ws._drop_zero = torch.zeros(ws.M, D, dtype=torch.float32, device=x_in.device)
        cls_top = bool(cls_top and N > 1 and g.depth >= 1)
        if cls_top and ws.training and B % 8:
            raise _lib.PolypMaeError("the cls-row top block needs a batch that is a multiple of 8 to train (16-byte k-major rows)")
        ws.cls_top = cls_top
        tc = None
        if cls_top and x_in.is_cuda:
            # a new workspace fills its cls-row index tables with launches on THIS stream: they must be enqueued before the fork
            # below, or the other half's gather reads `rows` on its own stream before they are written (recycled allocator
            # memory then holds stale indices: an out-of-bounds gather)
            tc = self.top_compact(ws, g, k.act_dtype, x_in.device)
        # The forward has no second stream of its own work to share the CUs with, so the batch is cut into two halves
        # that run as independent chains on two streams: one half's GEMM tails / attention / LayerNorm fill the CUs
        # the other half's kernels leave idle (every op is per token or per (sample, head), and the halves write
        # disjoint row ranges of the same workspaces, so the backward sees one batch).
        main = torch.cuda.current_stream() if x_in.is_cuda else None
        nparts = min(k.SPLIT_FORWARD, B)
        split = nparts > 1 and main is not None and not torch.cuda.is_current_stream_capturing()
        if split:
            auxs = [k.aux_stream(x_in.device, j) for j in range(nparts - 1)]
            for aux in auxs:
                self.fork(main, aux)
            cuts = [B * j // nparts for j in range(nparts + 1)]
            parts = [((main if j == 0 else auxs[j - 1]), cuts[j], cuts[j + 1]) for j in range(nparts)]
        else:
            parts = [(None, 0, B)]
        # PM_BLOCK_CALLS=0: every kernel of a block as its own C call from Python (the same launches; A/B and a fallback)
        fast = k.BLOCK_CALLS and x_in.is_cuda
        if fast:
            lib = k.lib
            cache = ws._fwd_descs
            raw = [(st.cuda_stream if st is not None and st is not main else None) for st, _, _ in parts]
        x = x_in
        for i in range(g.depth):
            if before_block is not None:
                if split:
                    before_block(i, also=auxs)
                else:
                    before_block(i)
            bw, p = ws.block(i), W[i]
            top = cls_top and i == g.depth - 1
            dropped = drop is not None and drop[i]
            if fast and not top and not dropped:
                # one C call per (block, sample range): pm_vit_block_fwd issues the same seven launches from a descriptor that
                # is built once and kept (every buffer it names is persistent: workspace, flat parameters, bf16 shadow)
                for j, (st, b0, b1) in enumerate(parts):
                    key = (b0, b1, x.data_ptr(), p["attn.qkv.weight"].data_ptr(), p["norm1.weight"].data_ptr(), k.gemm_variant,
                           i >= keep_from)
                    ent = cache.get((i, j))
                    if ent is None or ent[0] != key:
                        ent = cache[(i, j)] = (key, self._fwd_desc(ws, bw, p, x, b0, b1, keep=i >= keep_from))
                    _lib.check(lib.pm_vit_block_fwd(ctypes.byref(ent[1]), raw[j] if raw[j] is not None else _stream()),
                               "pm_vit_block_fwd")
                x = bw.x_out
                continue
            if top and tc is None:
                tc = self.top_compact(ws, g, k.act_dtype, x.device)
            for st, b0, b1 in parts:
                r0, r1 = b0 * N, b1 * N
                with (torch.cuda.stream(st) if st is not None and st is not main else contextlib.nullcontext()):
                    self._attn_half(bw, p, x, b0, b1, N)
                    if top:  # the two gathers, then the rest of the block on the cls rows of these samples
                        idx = tc["rows"][b0:b1]
                        k.gather_rows(x.view(-1, D), idx, out=tc["x"][b0:b1])
                        k.gather_rows(bw.attn.view(-1, D), idx, out=tc["attn"][b0:b1])
                        self._mlp_half(p, [tc[n][b0:b1] for n in _MLP_HALF_BUFFERS], b1 - b0, i >= keep_from)
                    elif dropped:
                        self._mlp_half(p, [t[r0:r1] for t in (x, bw.attn, bw.x_mid, bw.ln2, bw.mean2, bw.rstd2, bw.h_pre, bw.h_act,
                                                              bw.x_out)], r1 - r0, i >= keep_from,
                                       drop=(drop_scales[i, 0, b0:b1], drop_scales[i, 1, b0:b1], ws._drop_zero[r0:r1], N))
                    else:
                        self._mlp_half(p, [t[r0:r1] for t in (x, bw.attn, bw.x_mid, bw.ln2, bw.mean2, bw.rstd2, bw.h_pre, bw.h_act,
                                                              bw.x_out)], r1 - r0, i >= keep_from)
            x = tc["x_out"] if top else bw.x_out
        if split:
            for aux in auxs:
                self.fork(aux, main)
        return x

    def _attn_half(self, bw: BlockWorkspace, p, x: torch.Tensor, b0: int, b1: int, N: int) -> None:
        """The first three launches of a block over samples [b0, b1) of the dense workspaces: LayerNorm1, qkv GEMM, attention."""
        k, g = self.k, self.g
        D = g.dim
        r0, r1, h0, h1 = b0 * N, b1 * N, b0 * g.heads * N, b1 * g.heads * N
        ln1 = bw.ln1[r0:r1]
        qkv = bw.qkv[r0:r1]
        k.layernorm_fwd(x[r0:r1], p["norm1.weight"], p["norm1.bias"], ln1, bw.mean1[r0:r1], bw.rstd1[r0:r1], r1 - r0, D)
        k.linear_fwd(ln1, p["attn.qkv.weight"], p["attn.qkv.bias"], qkv, r1 - r0, 3 * D, D)
        k.attention_fwd(qkv, bw.attn[r0:r1], bw.lse[h0:h1], b1 - b0, N, g.heads, g.dh)

    def _mlp_half(self, p, bufs, M: int, keep: bool, drop=None) -> None:
        """The last four launches of a block over M rows: proj + residual, LayerNorm2, fc1 + GELU, fc2 + residual.  bufs: the row
        ranges (_MLP_HALF_BUFFERS) of a BlockWorkspace and the block's input, or of the compact cls-row buffers.  keep: fc1 stores
        its pre-activation (a backward will run through this block).
        drop = (attention scales, MLP scales, zeros f32 [M, D], N) of these rows' samples: stochastic depth -- the two residual GEMMs
        add their branch to zeros and pm_drop_path_add makes x_mid = x + s * branch (and x_out) in place: six launches."""
        k, D, Hd = self.k, self.g.dim, self.g.hidden
        x, attn, x_mid, ln2, mean2, rstd2, h_pre, h_act, x_out = bufs
        s_attn, s_mlp, zero, N = drop if drop is not None else (None, None, None, 0)
        k.linear_fwd(attn, p["attn.proj.weight"], p["attn.proj.bias"], x_mid, M, D, D, EPI_RESIDUAL, resid=x if drop is None else zero)
        if drop is not None:
            k.drop_path_add(x, x_mid, x_mid, s_attn, M, N, D)
        k.layernorm_fwd(x_mid, p["norm2.weight"], p["norm2.bias"], ln2, mean2, rstd2, M, D)
        k.linear_fwd(ln2, p["mlp.fc1.weight"], p["mlp.fc1.bias"], h_act, M, Hd, D, EPI_GELU, aux=h_pre if keep else None)
        k.linear_fwd(h_act, p["mlp.fc2.weight"], p["mlp.fc2.bias"], x_out, M, D, Hd, EPI_RESIDUAL, resid=x_mid if drop is None else zero)
        if drop is not None:
            k.drop_path_add(x_mid, x_out, x_out, s_mlp, M, N, D)

    def _drop_plan(self, ws: StackWorkspace, drop_scales: Optional[torch.Tensor], drop_blocks: Optional[Sequence[bool]]):
        """Which blocks run with the scale table (a list of depth flags), None without a table; the table is checked here."""
        if drop_scales is None:
            return None
        depth = self.g.depth
        if (tuple(drop_scales.shape) != (depth, 2, ws.B) or drop_scales.dtype != torch.float32 or not drop_scales.is_contiguous()
                or not drop_scales.is_cuda):
            raise _lib.PolypMaeError(f"drop_scales must be a contiguous f32 [{depth}, 2, {ws.B}] tensor on the device "
                                     f"(got {drop_scales.dtype} {tuple(drop_scales.shape)})")
        if drop_blocks is None:
            return [True] * depth
        if len(drop_blocks) != depth:
            raise _lib.PolypMaeError(f"drop_blocks names {len(drop_blocks)} blocks, the stack has {depth}")
        return [bool(t) for t in drop_blocks]

    @staticmethod
    def top_compact(ws: StackWorkspace, g: StackGeom, act_dtype, dev) -> dict:
        """Compact [B, ...] buffers of the top block's cls rows (forward saves + the head's gradient), kept on the workspace."""
        tc = ws._top_c
        if tc is None:
            B, N, D, Hd, f32 = ws.B, ws.N, g.dim, g.hidden, torch.float32
            e = lambda *s, dt=act_dtype: torch.empty(*s, dtype=dt, device=dev)
            rows = torch.arange(B, dtype=torch.int32, device=dev) * N          # (built on the device: no host copy, no sync)
            inv = torch.full((B * N,), -1, dtype=torch.int32, device=dev)
            inv[rows.long()] = torch.arange(B, dtype=torch.int32, device=dev)
            tc = ws._top_c = dict(
                rows=rows, inv=inv, x=e(B, D, dt=f32), attn=e(B, D), x_mid=e(B, D, dt=f32), ln2=e(B, D), mean2=e(B, dt=f32),
                rstd2=e(B, dt=f32), h_pre=e(B, Hd), h_act=e(B, Hd), x_out=e(B, D, dt=f32), dx=e(B, D, dt=f32), dx_act=e(B, D))
        return tc

    def _fwd_desc(self, ws: StackWorkspace, bw: BlockWorkspace, p, x: torch.Tensor, b0: int, b1: int, keep: bool = True):
        """pm_block_fwd_desc of block `bw` for samples [b0, b1): every pointer at the first row of the range.  keep = False:
        h_pre = NULL (the pre-activation of fc1 is not stored: no backward through this block)."""
        k, g = self.k, self.g
        N, D, Hd = ws.N, g.dim, g.hidden
        r0, h0 = b0 * N, b0 * g.heads * N
        a = lambda t, row, width: t.data_ptr() + row * width * t.element_size()
        v = lambda t: t.data_ptr() if t is not None else None
        return _lib.BlockFwdDesc(
            a(x, r0, D), a(bw.x_mid, r0, D), a(bw.x_out, r0, D), a(bw.ln1, r0, D), a(bw.mean1, r0, 1), a(bw.rstd1, r0, 1),
            a(bw.qkv, r0, 3 * D), a(bw.lse, h0, 1), a(bw.attn, r0, D), a(bw.ln2, r0, D), a(bw.mean2, r0, 1), a(bw.rstd2, r0, 1),
            a(bw.h_pre, r0, Hd) if keep else None, a(bw.h_act, r0, Hd),
            v(p["norm1.weight"]), v(p["norm1.bias"]), v(p["norm2.weight"]), v(p["norm2.bias"]),
            v(p["attn.qkv.weight"]), v(p["attn.proj.weight"]), v(p["mlp.fc1.weight"]), v(p["mlp.fc2.weight"]),
            v(p["attn.qkv.bias"]), v(p["attn.proj.bias"]), v(p["mlp.fc1.bias"]), v(p["mlp.fc2.bias"]),
            (b1 - b0) * N, b1 - b0, N, D, Hd, g.heads, k.act, k.gemm_variant, k.eps)

    def _block_scratch_bytes(self, M: int) -> Tuple[int, int]:
        """What pm_vit_block_bwd takes scratch for: the LayerNorm partial rows (main stream) and the slabs of a k-sliced grouped
        weight gradient (side stream; 0 when the library does not slice the group)."""
        k, D, Hd = self.k, self.g.dim, self.g.hidden
        return k._ln_bwd_bytes(M, D), k._need(("groupws", M, k.act, D, Hd), lambda: k.lib.pm_wgrad_group_workspace_bytes(
            k._shape_items(((D, Hd, False), (Hd, D, True), (D, D, False), (3 * D, D, True))), 4, M, k.act))

    def _bwd_desc(self, ws, bw, p, gr, xin, dx, dx_act, dmid, dmid_act, din, din_act, d_hidden, d_qkv, below_bias, acc, side, main,
                  ws_ln, ws_group):
        """(pm_block_bwd_desc, done event, objects to keep alive) of one block: the events are created once and reused.  ws_ln /
        ws_group: the main / side stream's scratch (ws_group None: the group is not k-sliced)."""
        k, g = self.k, self.g
        M, D, Hd = ws.M, g.dim, g.hidden
        v = lambda t: t.data_ptr() if t is not None else None
        need_ln, need = self._block_scratch_bytes(M)
        mk = lambda: torch.cuda.Event(enable_timing=bool(k.TIME_BLOCK_EVENTS))
        ev_fork, ev_done = mk(), mk()
        ev_fork.record(main)   # (materialises the hipEvent_t handles; re-recorded by every call)
        ev_done.record(main)
        two = not need and k.two_launch_group(M, ((D, Hd), (Hd, D), (D, D), (3 * D, D)))
        ev_fork2 = ev_done2 = side2 = None
        if two:
            side2 = k.side_stream2(dx.device)
            ev_fork2, ev_done2 = mk(), mk()
            ev_fork2.record(main)
            ev_done2.record(main)
        desc = _lib.BlockBwdDesc(
            v(xin), v(bw.x_mid), v(bw.ln1), v(bw.qkv), v(bw.attn), v(bw.ln2), v(bw.h_pre), v(bw.h_act), v(bw.mean1), v(bw.rstd1),
            v(bw.mean2), v(bw.rstd2), v(bw.lse), v(p["norm1.weight"]), v(p["norm2.weight"]), v(p["attn.qkv.weight"]),
            v(p["attn.proj.weight"]), v(p["mlp.fc1.weight"]), v(p["mlp.fc2.weight"]), v(dx), v(dx_act), v(dmid), v(dmid_act), v(din),
            v(din_act), v(d_hidden), v(d_qkv), v(ws.d_ln), v(ws.d_attn), v(ws.delta),
            v(gr["norm1.weight"]), v(gr["norm1.bias"]), v(gr["norm2.weight"]), v(gr["norm2.bias"]), v(gr["attn.qkv.weight"]),
            v(gr["attn.proj.weight"]), v(gr["mlp.fc1.weight"]), v(gr["mlp.fc2.weight"]), v(gr["attn.qkv.bias"]),
            v(gr["attn.proj.bias"]), v(gr["mlp.fc1.bias"]), v(below_bias),
            v(ws_ln), need_ln, v(ws_group), need,
            side.cuda_stream, None, ev_fork.cuda_event, ev_done.cuda_event,
            ws.B, ws.N, D, Hd, g.heads, k.act, k.gemm_variant, k.GROUP_BLOCKS_SLICED if need else k.GROUP_BLOCKS, acc,
            int(two), side2.cuda_stream if two else None, ev_fork2.cuda_event if two else None, ev_done2.cuda_event if two else None)
        return desc, (ev_done, ev_done2) if two else (ev_done,), (ev_fork, ev_fork2, ws_ln, ws_group)

    def backward(self, ws: StackWorkspace, x_in: torch.Tensor, W, G, dx: torch.Tensor, dx_act: torch.Tensor,
                 last_bias_grad_done: bool, trainable: Sequence[bool], need_input_grad: bool,
                 accumulate: Callable[[str, int], bool], on_block_done: Optional[Callable[[int], None]] = None,
                 prev_bias_grad: Optional[torch.Tensor] = None,
                 ends_pass: bool = True, defer_join: bool = False, drop_scales: Optional[torch.Tensor] = None,
                 drop_blocks: Optional[Sequence[bool]] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """dx / dx_act: gradient w.r.t. the stack output (f32 + act copy).  G[i][name] = f32 gradient
        tensors (vectors are += targets and must be zeroed or hold the running sum; matrices follow
        accumulate(name, i)).  `last_bias_grad_done`: the producer of dx already added colsum(dx) into the
        last block's fc2.bias gradient.  `prev_bias_grad`: bias gradient of the Linear that produced the
        stack input (receives colsum of the input gradient), if any.  `ends_pass`: nothing but a short tail follows this
        stack in the backward pass (the encoder; not the MAE decoder, whose weight gradients run beside the encoder's chain).
        `defer_join`: do not make the main stream wait for the last blocks' weight gradients here -- the caller still has
        main-stream work that does not read them (the embedding's backward) and calls `join_deferred(ws)` after it; the side
        stream's last launches then run beside that work instead of in front of it.
        `ws.cls_top` (left by the forward): dx / dx_act are the head's gradient on the B cls rows ([B, D]); the top block's backward
        then runs on those rows up to its attention (see _top_block_sparse).
        drop_scales / drop_blocks: what the forward got (stochastic depth).  The identity path carries the gradient unscaled and a
        branch receives s o dy, and every operation of a branch backward is linear per sample: a block that ran with the table goes
        kernel by kernel, with the act copy of its incoming gradient made by pm_drop_path_scale_cast with the MLP scales (fc2.bias
        gets the column sums of the scaled rows) and dmid_act made the same way with the attention scales (attn.proj.bias); whoever
        produced the f32 gradient is asked for neither the act copy nor that column sum -- the LayerNorm1 backward of the block above
        here, the caller for the top block: dx_act is then the buffer to fill, and `last_bias_grad_done` must be False.
        Returns (dx_in f32, dx_in act) or (None, None) when nothing below needs it."""
        k, g = self.k, self.g
        B, N, M, D, Hd = ws.B, ws.N, ws.M, g.dim, g.hidden
        drop = self._drop_plan(ws, drop_scales, drop_blocks)
        if drop and drop[-1] and last_bias_grad_done:
            raise _lib.PolypMaeError("stochastic depth: the top block's fc2.bias gradient is the column sum of the SCALED gradient; "
                                     "the caller must not have added the unscaled one")
        lowest = min([i for i, t in enumerate(trainable) if t], default=g.depth)
        main = torch.cuda.current_stream()
        pending: Dict[int, Tuple[torch.cuda.Event, ...]] = {}  # block -> side-stream event(s) after its last weight-gradient kernels

        def join(down_to: int):
            for j in sorted((j for j in pending if j >= down_to), reverse=True):
                for ev in pending.pop(j):
                    main.wait_event(ev)

        # PM_BLOCK_CALLS: fully trainable, grouped blocks go through pm_vit_block_bwd (one C call per block)
        fast = k.BLOCK_CALLS and dx.is_cuda and not torch.cuda.is_current_stream_capturing()
        dims = ((D, Hd), (Hd, D), (D, D), (3 * D, D))  # (n_out, n_in) of fc2, fc1, proj, qkv
        bcache = ws._bwd_descs
        ptr_of = lambda t: t.data_ptr() if t is not None else 0
        if fast:  # what a block call takes scratch for, from the arenas of the stream each launch goes to
            arena, main_key, (need_ln, need_group) = k._arena, _stream_key(main), self._block_scratch_bytes(M)
        for i in reversed(range(g.depth)):
            if i < lowest and not need_input_grad:
                join(0)
                return None, None
            bw, p, gr, tr = ws.block(i), W[i], G[i], trainable[i]
            xin = x_in if i == 0 else ws.block(i - 1).x_out
            # the bias gradient of the Linear below this block (fc2 of block i-1, or the caller's): LayerNorm1' adds colsum(d x_in) to it
            below_bias = (G[i - 1]["mlp.fc2.bias"] if trainable[i - 1] else None) if i > 0 else prev_bias_grad
            need_dx_in = need_input_grad or i > lowest
            o = i & 1
            dmid, din = ws.dx[o], ws.dx[o ^ 1]  # f32 residual gradients: main stream only, ping-pong (in-place add is fine)
            d_hidden, d_qkv = ws.d_hidden[o], ws.d_qkv[o]
            # act copies rotate through five buffers, two steps per block: wgrad(fc2) / wgrad(proj) of this block read
            # the incoming one / dmid_act on the side stream, possibly until the main stream has finished block i-1,
            # which writes the next two slots.
            pin = next((j for j in range(5) if dx_act is ws.dx_act[j]), 4)
            dmid_act, din_act = ws.dx_act[(pin + 1) % 5], ws.dx_act[(pin + 2) % 5]
            join(i + 2)  # block i overwrites what the side stream read for block i+2
            if i == g.depth - 1 and ws.cls_top:
                ev_last = self._top_block_sparse(ws, bw, p, gr, xin, dx, dx_act, last_bias_grad_done, dmid, din, din_act,
                                                 d_qkv, below_bias, lambda n: accumulate(n, i), main, on_block_done, i, tr)
                if ev_last is not None:
                    pending[i] = ev_last
                dx, dx_act = din, din_act
                continue
            dropped = drop is not None and drop[i]
            below_dropped = drop is not None and i > 0 and drop[i - 1]   # block i-1 makes its own act copy and fc2.bias gradient
            if dropped:
                k.drop_path_scale_cast(dx, drop_scales[i, 1], dx_act, gr["mlp.fc2.bias"] if tr else None, M, N, D)
            elif i == g.depth - 1 and not last_bias_grad_done and tr:
                k.colsum(dx, gr["mlp.fc2.bias"], M, D)
            # Weight gradients run on a side stream, concurrently with the dgrad chain on the main stream: the two
            # kernels' blocks share the CUs out of phase, so one's epilogue / partial last round hides under the
            # other's k-loop (both read the same dY; every buffer the side stream reads stays untouched until the
            # join below).
            side = k.side_stream(main.device) if tr else None
            # One grouped launch for the block's four weight gradients (full-K tiles, no split-K slabs), issued once the
            # whole dgrad chain of the block is enqueued; it runs beside block i-1's chain.  A grouped launch carries the qkv / fc1
            # bias gradients (column sums of its dY); otherwise they are k.colsum launches on the side stream.
            grouped = tr and (not ends_pass or i - lowest >= k.UNGROUP_TAIL) and k.can_group_wgrad(M, dims)
            if grouped and fast and not dropped and not below_dropped:
                # the whole block in ONE C call (pm_vit_block_bwd): the same launches, the same fork / done events, from a
                # descriptor built once per block and kept (every buffer it names is persistent)
                acc = (int(accumulate("attn.qkv.weight", i)) | int(accumulate("attn.proj.weight", i)) << 1 |
                       int(accumulate("mlp.fc1.weight", i)) << 2 | int(accumulate("mlp.fc2.weight", i)) << 3)
                ws_ln = arena.get(main_key, need_ln, main.device)
                ws_group = arena.get(_stream_key(side), need_group, main.device) if need_group else None
                key = (dx.data_ptr(), dx_act.data_ptr(), xin.data_ptr(), gr["attn.qkv.weight"].data_ptr(),
                       p["attn.qkv.weight"].data_ptr(), gr["norm1.weight"].data_ptr(),
                       below_bias.data_ptr() if below_bias is not None else 0, acc, k.gemm_variant, k.GROUP_BLOCKS, k.GROUP_BLOCKS_SLICED, k.TWO_GROUPS, k.TIME_BLOCK_EVENTS,
                       ws_ln.data_ptr(), ptr_of(ws_group))  # (scratch is replaced when it grows)
                ent = bcache.get(i)
                if ent is None or ent[0] != key:
                    ent = bcache[i] = (key,) + self._bwd_desc(ws, bw, p, gr, xin, dx, dx_act, dmid, dmid_act, din, din_act,
                                                              d_hidden, d_qkv, below_bias, acc, side, main, ws_ln, ws_group)
                _, desc, evs_done, keep = ent
                _lib.check(k.lib.pm_vit_block_bwd(ctypes.byref(desc), _stream()), "pm_vit_block_bwd")
                pending[i] = evs_done
                if on_block_done is not None:
                    if len(evs_done) == 2:  # the block's gradients are final behind BOTH launches: the later one's stream
                        last = k.side_stream2(main.device)
                        last.wait_event(evs_done[0])
                    else:
                        last = side
                    with torch.cuda.stream(last):
                        on_block_done(i)
                dx, dx_act = din, din_act
                continue
            # ---- MLP branch ----
            if tr and not grouped:
                self.fork(main, side)
                with torch.cuda.stream(side):
                    k.linear_wgrad(dx_act, bw.h_act, gr["mlp.fc2.weight"], M, D, Hd, accumulate("mlp.fc2.weight", i))
            # the launcher's two-launch schedule, kernel by kernel: (fc2, fc1) behind dfc2 on the side stream, (proj, qkv) behind
            # the attention backward on the second one
            two = grouped and k.two_launch_group(M, dims)
            group_mlp = [(dx_act, bw.h_act, gr["mlp.fc2.weight"], accumulate("mlp.fc2.weight", i)),
                         (d_hidden, bw.ln2, gr["mlp.fc1.weight"], accumulate("mlp.fc1.weight", i), gr["mlp.fc1.bias"])] if grouped else None
            ev_mlp = None

            def wgrad_behind_dfc2():
                nonlocal ev_mlp
                self.fork(main, side)
                with torch.cuda.stream(side):
                    if not grouped:
                        k.linear_wgrad(d_hidden, bw.ln2, gr["mlp.fc1.weight"], M, Hd, D, accumulate("mlp.fc1.weight", i))
                        k.colsum(d_hidden, gr["mlp.fc1.bias"], M, Hd)
                    elif two:
                        if not k.wgrad_group(group_mlp, M):
                            raise _lib.PolypMaeError("pm_wgrad_group refused a group that two_launch_group admitted")
                        ev_mlp = torch.cuda.Event()
                        ev_mlp.record(side)

            self._mlp_dgrad(p, gr if tr else None, M, dx, dx_act, bw.h_pre, d_hidden, ws.d_ln, bw.x_mid, bw.mean2, bw.rstd2, dmid, dmid_act,
                            wgrad_behind_dfc2 if tr else None, drop=(drop_scales[i, 0], N) if dropped else None)
            # ---- attention branch ----
            if tr and not grouped:
                self.fork(main, side)
                with torch.cuda.stream(side):
                    k.linear_wgrad(dmid_act, bw.attn, gr["attn.proj.weight"], M, D, D, accumulate("attn.proj.weight", i))
            k.linear_dgrad(dmid_act, p["attn.proj.weight"], ws.d_attn, M, D, D)
            k.attention_bwd(bw.qkv, bw.attn, ws.d_attn, bw.lse, ws.delta, d_qkv, B, N, g.heads, g.dh)
            if tr:
                last = k.side_stream2(main.device) if two else side
                self.fork(main, last)
                with torch.cuda.stream(last):
                    if grouped:
                        group_attn = [(dmid_act, bw.attn, gr["attn.proj.weight"], accumulate("attn.proj.weight", i)),
                                      (d_qkv, bw.ln1, gr["attn.qkv.weight"], accumulate("attn.qkv.weight", i), gr["attn.qkv.bias"])]
                        ok = k.wgrad_group(group_attn, M, whole_k=True) if two else k.wgrad_group(group_mlp + group_attn, M)
                        if not ok:
                            raise _lib.PolypMaeError("pm_wgrad_group refused a group that can_group_wgrad admitted")
                    else:
                        k.colsum(d_qkv, gr["attn.qkv.bias"], M, 3 * D)
                        k.linear_wgrad(d_qkv, bw.ln1, gr["attn.qkv.weight"], M, 3 * D, D, accumulate("attn.qkv.weight", i))
                    # no join here: the main stream runs on into block i-1 and waits for these events only before
                    # block i-2.  The block's matrix gradients are final behind the last launch of each stream.
                    ev_last = torch.cuda.Event()
                    ev_last.record(last)
                    pending[i] = (ev_mlp, ev_last) if two else (ev_last,)
                    if on_block_done is not None:
                        if two:
                            last.wait_event(ev_mlp)
                        on_block_done(i)
            if not (need_dx_in or tr):
                join(0)
                return None, None
            self._qkv_dgrad_ln1(p, gr if tr else None, M, d_qkv, ws.d_ln, xin, bw.mean1, bw.rstd1, dmid, din,
                                None if below_dropped else din_act, None if below_dropped else below_bias)
            dx, dx_act = din, din_act
            if on_block_done is not None and not tr:
                on_block_done(i)
        if defer_join:
            ws._deferred_join = [ev for j in sorted(pending, reverse=True) for ev in pending.pop(j)]
        else:
            join(0)
        return dx, dx_act

    def _mlp_dgrad(self, p, gr, M: int, dy, dy_act, h_pre, d_hidden, d_ln, x_mid, mean2, rstd2, dmid, dmid_act,
                   behind_dfc2: Optional[Callable[[], None]] = None, drop=None) -> None:
        """The dgrad chain of a block's MLP branch over M rows, dense or compact: dfc2 + dGELU (dy_act -> d_hidden), dfc1 (-> d_ln),
        LayerNorm2' (+ the residual gradient dy -> dmid f32, dmid_act).  gr: the block's gradient tensors, None when it is frozen
        (LayerNorm2' then leaves out d gamma, d beta and the proj bias gradient it carries).  behind_dfc2(): the caller's weight
        gradients that read d_hidden, enqueued between dfc2 and dfc1 -- on which stream is its business.
        drop = (attention scales, N): stochastic depth -- dy_act came in scaled by the MLP scales; LayerNorm2' makes dmid alone, and
        dmid_act and the proj bias gradient are the attention branch's view of it (pm_drop_path_scale_cast)."""
        k, D, Hd = self.k, self.g.dim, self.g.hidden
        k.linear_dgrad(dy_act, p["mlp.fc2.weight"], d_hidden, M, D, Hd, EPI_DGELU, aux=h_pre)
        if behind_dfc2 is not None:
            behind_dfc2()
        k.linear_dgrad(d_hidden, p["mlp.fc1.weight"], d_ln, M, Hd, D)
        proj_bias = gr["attn.proj.bias"] if gr else None
        k.layernorm_bwd(d_ln, x_mid, p["norm2.weight"], mean2, rstd2, dy, dmid, dmid_act if drop is None else None,
                        gr["norm2.weight"] if gr else None, gr["norm2.bias"] if gr else None, proj_bias if drop is None else None, M, D)
        if drop is not None:
            k.drop_path_scale_cast(dmid, drop[0], dmid_act, proj_bias, M, drop[1], D)

    def _qkv_dgrad_ln1(self, p, gr, M: int, d_qkv, d_ln, xin, mean1, rstd1, dmid, din, din_act, below_bias) -> None:
        """The tail of a block's backward over M rows: qkv dgrad (d_qkv -> d_ln), LayerNorm1' (+ dmid -> din f32, din_act; colsum of
        din into below_bias).  gr as in _mlp_dgrad."""
        k, D = self.k, self.g.dim
        k.linear_dgrad(d_qkv, p["attn.qkv.weight"], d_ln, M, 3 * D, D)
        k.layernorm_bwd(d_ln, xin, p["norm1.weight"], mean1, rstd1, dmid, din, din_act,
                        gr["norm1.weight"] if gr else None, gr["norm1.bias"] if gr else None, below_bias, M, D)

    def _top_block_sparse(self, ws, bw, p, gr, xin, dx, dx_act, last_bias_grad_done, dmid, din, din_act, d_qkv, below_bias,
                          acc, main, on_block_done, i, tr):
        """Backward of the top block of a classifier that reads the cls row only (forward: the cls_top block of BlockStack.forward).
        dx / dx_act are the head's gradient on the B cls rows ([B, D], pm_vit_head_bwd with N = 1); the block's saves behind the
        attention are compact too.
        The MLP branch and the proj Linear -- dfc2 + dGELU, dfc1, LayerNorm2', proj dgrad, the fc2 / fc1 / proj weight gradients -- run at
        M = B; d mid and d attn are scattered into zero-filled dense buffers (a zero row of dY adds nothing anywhere, and the residual
        path adds zero to zero), and from the attention backward on -- which spreads the gradient over all keys -- the block is dense:
        qkv weight gradient on the side stream, qkv dgrad, LayerNorm1'.  The reference's autograd multiplies those zeros; skipping them
        is the same kind of identity as embedding only the kept patches in MAE."""
        k, g = self.k, self.g
        tc = self.top_compact(ws, g, k.act_dtype, dx.device)
        B, N, M, D, Hd = ws.B, ws.N, ws.M, g.dim, g.hidden
        R = B
        e = lambda *s, dt=k.act_dtype: torch.empty(*s, dtype=dt, device=dx.device)
        dxc, dxac = dx.view(R, D), dx_act.view(R, D)
        if tr and not last_bias_grad_done:
            k.colsum(dxc, gr["mlp.fc2.bias"], R, D)
        # ---- MLP branch on the live rows: its weight gradients are a few tiles each, on the main stream behind dfc2
        d_hidden_c, d_ln_c, dmid_c, dmid_act_c, d_attn_c = e(R, Hd), e(R, D), e(R, D, dt=torch.float32), e(R, D), e(R, D)

        def wgrad_behind_dfc2():
            k.linear_wgrad(dxac, tc["h_act"], gr["mlp.fc2.weight"], R, D, Hd, acc("mlp.fc2.weight"))
            k.linear_wgrad(d_hidden_c, tc["ln2"], gr["mlp.fc1.weight"], R, Hd, D, acc("mlp.fc1.weight"))
            k.colsum(d_hidden_c, gr["mlp.fc1.bias"], R, Hd)

        self._mlp_dgrad(p, gr if tr else None, R, dxc, dxac, tc["h_pre"], d_hidden_c, d_ln_c, tc["x_mid"], tc["mean2"], tc["rstd2"],
                        dmid_c, dmid_act_c, wgrad_behind_dfc2 if tr else None)
        # ---- proj on the live rows, then dense again for the attention backward
        if tr:
            k.linear_wgrad(dmid_act_c, tc["attn"], gr["attn.proj.weight"], R, D, D, acc("attn.proj.weight"))
        k.linear_dgrad(dmid_act_c, p["attn.proj.weight"], d_attn_c, R, D, D)
        k.scatter_rows_zero(dmid_c, tc["inv"], dmid.view(M, D))
        k.scatter_rows_zero(d_attn_c, tc["inv"], ws.d_attn.view(M, D))
        k.attention_bwd(bw.qkv, bw.attn, ws.d_attn, bw.lse, ws.delta, d_qkv, B, N, g.heads, g.dh)
        ev_last = None
        if tr:
            side = k.side_stream(main.device)
            self.fork(main, side)
            with torch.cuda.stream(side):
                k.colsum(d_qkv, gr["attn.qkv.bias"], M, 3 * D)
                k.linear_wgrad(d_qkv, bw.ln1, gr["attn.qkv.weight"], M, 3 * D, D, acc("attn.qkv.weight"))
                ev_last = torch.cuda.Event()
                ev_last.record(side)
                if on_block_done is not None:
                    on_block_done(i)
        self._qkv_dgrad_ln1(p, gr if tr else None, M, d_qkv, ws.d_ln, xin, bw.mean1, bw.rstd1, dmid, din, din_act, below_bias)
        if not tr and on_block_done is not None:
            on_block_done(i)
        return (ev_last,) if ev_last is not None else None

    @staticmethod
    def join_deferred(ws: StackWorkspace) -> None:
        """Make the current stream wait for the weight-gradient launches a backward(..., defer_join=True) left running."""
        main = torch.cuda.current_stream()
        for ev in ws._deferred_join:
            main.wait_event(ev)
        ws._deferred_join = []
