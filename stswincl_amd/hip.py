"""ctypes binding of libstswin_hip.so (the C ABI declared in include/stswin_hip.h).

There is NO fallback: every wrapper raises if the library is missing or a kernel reports an error, and
every wrapper demands CUDA (ROCm) tensors.  PyTorch is used only for device memory and the stream handle.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from typing import Optional

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("STSWIN_HIP_LIB") or os.path.join(_ROOT, "stswincl_amd", "lib", "libstswin_hip.so")   # override: A/B of two builds in one process pool (tools/)
HEADER_PATH = os.path.join(_ROOT, "include", "stswin_hip.h")
_lib: Optional[ctypes.CDLL] = None

_c_int, _c_float, _c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p        # element types of the host arrays some entry points take


class StswinHipError(RuntimeError):
    pass


_C_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}


def _c_value(name: str, expr: str) -> int:
    """Value of a #define: integer literals (optional `u`), `<<`, `*`, `+`, `-` and parentheses - anything else raises.  The constants
    cross the ABI in `int` parameters, so bit 31 is the sign bit."""
    tokens = re.findall(r"0[xX][0-9a-fA-F]+|\d+|<<|[-+*()]|\S", re.sub(r"(?<=[0-9a-fA-F])[uU]\b", "", expr))
    if not tokens or not all(re.fullmatch(r"0[xX][0-9a-fA-F]+|\d+|<<|[-+*()]", t) for t in tokens):
        raise StswinHipError(f"{HEADER_PATH}: cannot evaluate `#define STSWIN_{name} {expr.strip()}`")
    try:
        v = int(eval(" ".join(tokens), {"__builtins__": {}}))       # (digits, shifts, products, sums and parentheses only: checked above)
    except (SyntaxError, TypeError) as e:
        raise StswinHipError(f"{HEADER_PATH}: cannot evaluate `#define STSWIN_{name} {expr.strip()}`") from e
    return v - (1 << 32) if v >= 1 << 31 else v


@functools.lru_cache(maxsize=None)
def _header():
    """include/stswin_hip.h, read once per process -> (prototypes {symbol: (restype, [argtypes])}, constants {NAME: value} of the
    `#define STSWIN_NAME value` lines).  A parameter is a pointer (anything with a `*`: c_void_p) or an optionally const int / long /
    float / double; whatever else appears is an error, never an int by default."""
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"\b(int|long)\s+(stswin_\w+)\s*\(([^()]*)\)\s*;", text):
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            if "*" in p:
                argtypes.append(ctypes.c_void_p)
            elif len(words) == 2 and words[0] in _C_TYPES:
                argtypes.append(_C_TYPES[words[0]])
            else:
                raise StswinHipError(f"{HEADER_PATH}: {name}: cannot bind parameter `{p.strip()}`")
        protos[name] = (_C_TYPES[ret], argtypes)
    unparsed = set(re.findall(r"\b(stswin_\w+)\s*\(", text)) - set(protos)
    if unparsed:
        raise StswinHipError(f"{HEADER_PATH}: cannot bind the declaration of {sorted(unparsed)}")
    consts = {name: _c_value(name, expr) for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+STSWIN_(\w+)[ \t]+(\S.*)$", text, flags=re.M)}
    return protos, consts


# GF_* (stswin_gemm_nt flags), TN_* (bits of stswin_gemm_tn's `splits`, TN_GROUP_DECLINED), VAR_* (stswin_last_variant codes) and
# OHEM_WORK_BYTES are the header's STSWIN_* #defines without the prefix: hip.GF_GELU == STSWIN_GF_GELU, ...
globals().update(_header()[1])


def declared_symbols():
    """Every entry point include/stswin_hip.h declares."""
    return sorted(_header()[0])


def load() -> ctypes.CDLL:
    """dlopen the library, check that it exports the whole declared ABI and give every entry point the restype and argtypes of its
    prototype (works without a GPU).  ctypes then converts plain ints / floats / None per parameter and refuses a wrong argument
    count or a float where an integer is declared."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StswinHipError(f"{LIB_PATH} not found: run `python __graft_entry__.py` (build()) first; "
                             "stswincl_amd has no CPU or eager fallback")
    lib = ctypes.CDLL(LIB_PATH)
    protos = _header()[0]
    missing = [s for s in sorted(protos) if not hasattr(lib, s)]
    if missing and not os.environ.get("STSWIN_HIP_LIB"):     # (an older build named for an A/B run may lack new entries)
        raise StswinHipError(f"libstswin_hip.so lacks declared symbols: {missing}")
    for s, (restype, argtypes) in protos.items():
        if s not in missing:
            fn = getattr(lib, s)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def tuning_build() -> bool:
    """True when the loaded library was built with STSWIN_TUNING=1 (A/B-only kernel variants and the in-kernel diagnosis switches)."""
    return bool(load().stswin_tuning_build())


def tn_fused_holds() -> int:
    """Outstanding holds on the fused split-K combine of stswin_gemm_tn (0 = fused where it applies)."""
    return int(load().stswin_tn_fused_hold(0))


class TnFusedHold:
    """While alive (until release()), weight-gradient GEMMs use the separate split-K combine pass instead of the one fused into the
    launch.  Refcounted inside the library (include/stswin_hip.h, stswin_tn_fused_hold): several holders, any order of release, and a
    holder dropped without release() gives its hold back when it is collected."""

    def __init__(self):
        import weakref
        lib = load()
        lib.stswin_tn_fused_hold(1)
        self._fin = weakref.finalize(self, lib.stswin_tn_fused_hold, -1)

    def release(self):
        self._fin()            # (idempotent: a finalizer runs once)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise StswinHipError(f"{what} failed with code {rc}")


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return 0
    if t.dtype == torch.float32:
        return 1
    raise StswinHipError(f"unsupported dtype {t.dtype}")


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device address of t for a pointer parameter (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise StswinHipError("stswincl_amd ops need tensors on the GPU (no CPU path exists)")
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    # the raw handle of the calling thread's current stream on the current device: torch.cuda.current_stream() builds a Stream
    # object per call (9 us, ~460 calls per training step = 4 ms of host time); the private accessor is 20x cheaper
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major 2-D view"
    return t.stride(0)


def _device(d) -> torch.device:
    """torch.device(d) with "cuda" resolved to the current device: the key of the per-device caches below."""
    d = torch.device(d)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


# ----------------------------------------------------------------------------------------------- zero arena
# Accumulators that the kernels add into (BatchNorm / LayerNorm statistic sums, bias gradients, CE counters) must start at
# zero; a fill launch per buffer costs ~4.5 us of GPU time and the training step needs ~80 of them.  zeros() hands out
# 64-byte aligned slices of one zero-filled block per device instead: ONE fill per block (4 M floats), a fresh block when
# the current one is used up or when arena_reset() is called (model forward: once per step).  A slice is handed out
# once and never recycled - the block is freed when its last slice dies - so nothing can observe stale contents.
_ARENA_FLOATS = 1 << 22
_ARENA_MAX_REQUEST = 0 if os.environ.get("STSWIN_NO_ARENA") == "1" else 1 << 18      # (switch for A/B runs)
_ARENAS = {}


def arena_reset(device=None) -> None:
    """Drop the current block(s): the next zeros() starts a fresh one (called at the start of a model forward so that a
    step's forward and backward share one fill and a long-lived slice does not pin a mostly unused block for ever)."""
    if device is None:
        _ARENAS.clear()
    else:
        _ARENAS.pop(_device(device), None)


def zeros(*shape, device) -> torch.Tensor:
    """fp32 zeros of the given shape: a slice of the device's zero arena (small requests) or torch.zeros (large ones)."""
    if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
        shape = tuple(shape[0])
    n = 1
    for d in shape:
        n *= int(d)
    if n > _ARENA_MAX_REQUEST or n == 0:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    device = _device(device)
    st = _ARENAS.get(device)
    need = (n + 15) // 16 * 16
    if st is None or st[1] + need > _ARENA_FLOATS:
        st = [torch.zeros(_ARENA_FLOATS, dtype=torch.float32, device=device), 0]
        _ARENAS[device] = st
    out = st[0][st[1]:st[1] + n].view(shape)
    st[1] += need
    return out


# ----------------------------------------------------------------------------------------------- scratch for deterministic sums
# Kernels that sum over workgroups store per-workgroup partial vectors into caller-owned scratch and a fold kernel adds them in a
# fixed order (include/stswin_hip.h, "deterministic cross-workgroup sums").  One buffer per device: every use is write-then-read on
# the launch stream and kernels of a stream run in order.  It only ever grows (warm-up steps size it before a hipGraph capture).
_SCRATCH = {}
_SCRATCH_RETIRED = []        # superseded (smaller) scratch blocks: see scratch()
_DEFER = [False, 0]          # [folds are being queued (deferred_folds), bump offset into the scratch buffer]
_CAPTURED = [False]          # a hipGraph capture has happened in this process (note_capture)


def note_capture() -> None:
    """Tell the scratch allocator that a hipGraph has been (or is being) captured: from now on superseded scratch blocks are retired,
    not freed (a captured kernel node keeps the address it was captured with).  scratch() also sets it when it sees a capture."""
    _CAPTURED[0] = True


def scratch(device, floats: int) -> torch.Tensor:
    device = _device(device)
    floats = (int(floats) + 63) // 64 * 64
    t = _SCRATCH.get(device)
    off = _DEFER[1] if _DEFER[0] else 0
    if not _CAPTURED[0] and device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        _CAPTURED[0] = True
    if t is None or t.numel() < off + floats:
        if _DEFER[0] and off > 0:            # queued folds still read the regions handed out so far: run them, then start over
            _check(load().stswin_fold_flush(_stream()), "fold_flush")
            _DEFER[1] = off = 0
        if t is None or t.numel() < floats:
            if t is not None and torch.cuda.is_current_stream_capturing():
                raise StswinHipError("scratch buffer would have to grow during a hipGraph capture: run the step once before capturing")
            if t is not None and _CAPTURED[0]:
                # A hipGraph captured earlier may still write and read the old block on every replay (its address is baked into the
                # graph's kernel arguments): superseded blocks are kept alive, never handed back to the caching allocator - but only
                # once a capture has happened in this process (note_capture(), called by whoever captures: bench.py, the tests);
                # before that nothing can refer to the old block and it is simply freed (round-4 advisor)
                _SCRATCH_RETIRED.append(t)
            # geometric growth: a run of increasing requests re-allocates O(log) times and retains at most ~2x the final size
            t = torch.empty(max(floats, 2 * (t.numel() if t is not None else 0), 1 << 23), dtype=torch.float32, device=device)
            _SCRATCH[device] = t
    if _DEFER[0]:
        _DEFER[1] = off + floats
        return t[off:off + floats]
    return t


class deferred_folds:
    """with deferred_folds() as d: the fixed-order folds of the kernels called inside (LayerNorm / bias-gradient / attention partial
    sums) are queued and launched together by d.flush() or at the end of the block - legal when none of their results is read
    in between (a Swin block's backward: they are all parameter gradients).  Every call gets its own region of the scratch buffer."""

    def __enter__(self):
        _check(load().stswin_fold_defer(1, _stream()), "fold_defer")
        _DEFER[0], _DEFER[1] = True, 0
        return self

    def flush(self):
        _check(load().stswin_fold_flush(_stream()), "fold_flush")
        _DEFER[1] = 0

    def abort(self):
        """Leave the deferred mode after an error inside the block (what was queued is still launched: its scratch is intact)."""
        _DEFER[0], _DEFER[1] = False, 0
        load().stswin_fold_defer(0, _stream())

    def __exit__(self, *exc):
        _DEFER[0], _DEFER[1] = False, 0
        _check(load().stswin_fold_defer(0, _stream()), "fold_defer")
        return False


# ----------------------------------------------------------------------------------------------- live profiling
# bench.py brackets every launch of the dominant kernels with HIP events recorded on the launch stream (torch's
# current stream IS the stream the kernels are launched on) and reads them back after the timed region.
# Two event records per launch cost ~1.7 ms of host time per training step (480 spans), which would make the timed
# region launch-bound; `stride` > 1 brackets one launch in `stride`.  WHICH ones rotates with the step (profile_step(k), called by
# the caller before step k): launch number n of a kernel family inside step k is timed iff (n + k) % stride == 0, so over `stride`
# steps every launch site of the step is timed exactly once and the average is the exact per-site average - not a sample whose
# composition changes whenever a launch is added or removed elsewhere (a seeded random choice moved the reported gemm_nt
# fraction by +-0.01 between trees with identical gemm_nt launches).  Without profile_step the choice is the seeded random one.
_PROFILE = None
_PROFILE_STRIDE = 1
_PROFILE_COUNT = {}
_PROFILE_STEP_COUNT = None            # per-step launch numbers (rotating mode) or None (random mode)
_PROFILE_OFFSET = 0
_PROFILE_RNG = None
_PROFILE_ALWAYS = ("contrast_",)      # kernels launched once per step: every launch is timed


def profile_begin(stride: int = 1):
    global _PROFILE, _PROFILE_STRIDE, _PROFILE_COUNT, _PROFILE_RNG, _PROFILE_STEP_COUNT, _PROFILE_OFFSET
    import random
    _PROFILE, _PROFILE_STRIDE, _PROFILE_COUNT, _PROFILE_RNG = {}, max(1, int(stride)), {}, random.Random(12345)
    _PROFILE_STEP_COUNT, _PROFILE_OFFSET = None, 0


def profile_step(k: int):
    """Start of timed step k: switch to (or stay in) the rotating choice of timed launches."""
    global _PROFILE_STEP_COUNT, _PROFILE_OFFSET
    if _PROFILE is not None:
        _PROFILE_STEP_COUNT, _PROFILE_OFFSET = {}, int(k) % _PROFILE_STRIDE


def profile_end():
    """-> {kernel: dict(launches, sampled, ms_total, ms_avg, work)}: ms_total / work cover the `sampled` launches that
    were bracketed by events (work = their algorithmic flops or bytes), `launches` counts every launch."""
    global _PROFILE
    prof, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    out = {}
    for name, recs in (prof or {}).items():
        ms = sum(a.elapsed_time(b) for a, b, _ in recs)
        out[name] = dict(launches=_PROFILE_COUNT.get(name, len(recs)), sampled=len(recs), ms_total=ms,
                         ms_avg=ms / max(len(recs), 1), work=sum(w for _, _, w in recs))
    return out


_SHAPE_NAMES = os.environ.get("STSWIN_SHAPE_PROFILE", "0") == "1"   # tools/shape_profile.py: one span name per GEMM shape


class _Span:
    def __init__(self, name, work):
        self.name, self.work = name, work

    def __enter__(self):
        self.a = None
        if _PROFILE is not None:
            n = _PROFILE_COUNT.get(self.name, 0)
            _PROFILE_COUNT[self.name] = n + 1
            if _PROFILE_STEP_COUNT is not None:
                m = _PROFILE_STEP_COUNT.get(self.name, 0)
                _PROFILE_STEP_COUNT[self.name] = m + 1
                pick = (m + _PROFILE_OFFSET) % _PROFILE_STRIDE == 0
            else:
                pick = _PROFILE_RNG.random() * _PROFILE_STRIDE < 1.0
            if _PROFILE_STRIDE == 1 or self.name.startswith(_PROFILE_ALWAYS) or pick:
                self.a = torch.cuda.Event(enable_timing=True)
                self.a.record()
        return self

    def cancel(self):
        """Nothing was launched inside the span (a declined grouped launch): no sample, and the launch / per-step site numbers
        __enter__ handed out go back, so that the family's launch count and the rotation of timed sites are those of the launches
        that did happen (the round-5 line counted a declined group as a launch and credited its work to the next sample)."""
        if _PROFILE is not None and not getattr(self, "_cancelled", False):
            self._cancelled = True
            _PROFILE_COUNT[self.name] = _PROFILE_COUNT.get(self.name, 1) - 1
            if _PROFILE_STEP_COUNT is not None and self.name in _PROFILE_STEP_COUNT:
                _PROFILE_STEP_COUNT[self.name] -= 1
        self.a = None

    def __exit__(self, *exc):
        if self.a is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _PROFILE.setdefault(self.name, []).append((self.a, b, self.work))
        return False


# ----------------------------------------------------------------------------------------------- row maps
def win_rowmap(B, T, H, W, ws, shift, f0=0, frames_total=None, device="cuda") -> torch.Tensor:
    frames_total = T if frames_total is None else frames_total
    m = torch.empty(B * T * H * W, dtype=torch.int32, device=device)
    _check(load().stswin_win_rowmap(_p(m), B, T, H, W, ws, shift, f0, frames_total, _stream()), "win_rowmap")
    return m


def win_move(x: torch.Tensor, B, T, H, W, ws, shift, direction: int, f0=0, frames_total=None) -> torch.Tensor:
    """direction 0: (B,Ftot,H*W,C) tokens -> (B*nW*T*N, C) window rows; 1: the inverse (into zeros)."""
    frames_total = T if frames_total is None else frames_total
    C = x.shape[-1]
    x = x.contiguous()
    if direction == 0:
        out = torch.empty(B * T * H * W, C, dtype=x.dtype, device=x.device)
    else:
        out = torch.zeros(B * frames_total * H * W, C, dtype=x.dtype, device=x.device)
    _check(load().stswin_win_move(_dt(x), _p(x), _p(out), B, T, H, W, C, ws, shift, f0, frames_total, direction,
                                  _stream()), "win_move")
    return out


def merge_rowmap(frames, H, W, device="cuda") -> torch.Tensor:
    m = torch.empty(4, frames * (H // 2) * (W // 2), dtype=torch.int32, device=device)
    _check(load().stswin_merge_rowmap(_p(m), frames, H, W, _stream()), "merge_rowmap")
    return m


def conv3x3_rowmap(frames, H, W, dilation, device="cuda") -> torch.Tensor:
    m = torch.empty(9, frames * H * W, dtype=torch.int32, device=device)
    _check(load().stswin_conv3x3_rowmap(_p(m), frames, H, W, dilation, _stream()), "conv3x3_rowmap")
    return m


def conv_rowmap(frames, Hin, Win, Hout, Wout, k, stride, pad, dil, inverse, device="cuda") -> torch.Tensor:
    n = frames * (Hin * Win if inverse else Hout * Wout)
    m = torch.empty(k * k, n, dtype=torch.int32, device=device)
    _check(load().stswin_conv_rowmap(_p(m), frames, Hin, Win, Hout, Wout, k, stride, pad, dil, 1 if inverse else 0,
                                     _stream()), "conv_rowmap")
    return m


def conv_pack(w: torch.Tensor, dt: torch.dtype, omap: torch.Tensor, imap: torch.Tensor, want_dgrad: bool = True):
    """(Cout,Cin,k,k) fp32 -> (fwd [cop][S*cip], dgrad [cip][S*cop] or None) in dtype dt; see include/stswin_hip.h."""
    co, ci, k, _ = w.shape
    S, cop, cip = k * k, omap.numel(), imap.numel()
    wf = w.detach().float().contiguous()
    fwd = torch.empty(cop, S * cip, dtype=dt, device=w.device)
    dg = torch.empty(cip, S * cop, dtype=dt, device=w.device) if want_dgrad else None
    _check(load().stswin_conv_pack(0 if dt == torch.bfloat16 else 1, _p(wf), _p(fwd), _p(dg), _p(omap), _p(imap), co, ci, S,
                                   cop, cip, _stream()), "conv_pack")
    return fwd, dg


def linear_pack(w: torch.Tensor, dt: torch.dtype, want_tr: bool = True):
    """nn.Linear weight [n][k] fp32 -> (W, W^T or None) in dtype dt, one launch."""
    n, k = w.shape
    wf = w.detach().float().contiguous()
    fwd = torch.empty(n, k, dtype=dt, device=w.device)
    tr = torch.empty(k, n, dtype=dt, device=w.device) if want_tr else None
    _check(load().stswin_linear_pack(0 if dt == torch.bfloat16 else 1, _p(wf), _p(fwd), _p(tr), n, k, _stream()), "linear_pack")
    return fwd, tr


def linear_pack_multi(entries, dt: torch.dtype):
    """entries: [(w fp32 [n][k], fwd [n][k], tr [k][n] or None)] -> re-pack all of them in place, 64 weights per launch."""
    lib, st = load(), _stream()
    for lo in range(0, len(entries), 64):
        ch = entries[lo:lo + 64]
        c = len(ch)
        ws = (_c_void_p * c)(*[e[0].data_ptr() for e in ch])
        fs = (_c_void_p * c)(*[e[1].data_ptr() for e in ch])
        ts = (_c_void_p * c)(*[(e[2].data_ptr() if e[2] is not None else 0) for e in ch])
        ns = (_c_int * c)(*[e[0].shape[0] for e in ch])
        ks = (_c_int * c)(*[e[0].shape[1] for e in ch])
        _check(lib.stswin_linear_pack_multi(0 if dt == torch.bfloat16 else 1, c, ws, fs, ts, ns, ks, st), "linear_pack_multi")


def conv_pack_multi(entries, dt: torch.dtype):
    """entries: [(w fp32 (co,ci,k,k), fwd, dgrad or None, omap, imap)] -> re-pack in place, 32 weights per launch."""
    lib, st = load(), _stream()
    for lo in range(0, len(entries), 32):
        ch = entries[lo:lo + 32]
        c = len(ch)
        arr = lambda i: (_c_void_p * c)(*[(e[i].data_ptr() if e[i] is not None else 0) for e in ch])  # noqa: E731
        ints = lambda f: (_c_int * c)(*[f(e) for e in ch])  # noqa: E731
        _check(lib.stswin_conv_pack_multi(0 if dt == torch.bfloat16 else 1, c, arr(0), arr(1), arr(2), arr(3), arr(4),
                                          ints(lambda e: e[0].shape[1]), ints(lambda e: e[0].shape[2] * e[0].shape[3]),
                                          ints(lambda e: e[3].numel()), ints(lambda e: e[4].numel()), st), "conv_pack_multi")


def stem_im2col(img: torch.Tensor, dtype: torch.dtype, Ho: int, Wo: int, ld: int = 192) -> torch.Tensor:
    """img fp32 NCHW [F][3][H][W] -> patches [F*Ho*Wo][ld] (7x7 / stride 2 / pad 3)."""
    F_, c, H, W = img.shape
    assert c == 3 and img.dtype == torch.float32 and img.is_contiguous()
    out = torch.empty(F_ * Ho * Wo, ld, dtype=dtype, device=img.device)
    _check(load().stswin_stem_im2col(_dt(out), _p(img), _p(out), ld, F_, H, W, Ho, Wo, _stream()), "stem_im2col")
    return out


def stem_s2d(img: torch.Tensor, dtype: torch.dtype):
    """img fp32 NCHW [F][3][H][W] -> (A, Hs, Ws): A = the [F*Hs*Ws][64] row view (row pitch 16: every row is the 4-record segment
    starting at its record) of the padded 2 x 2 space-to-depth image; see include/stswin_hip.h."""
    F_, c, H, W = img.shape
    assert c == 3 and img.dtype == torch.float32 and img.is_contiguous()
    Hs, Ws = (H - 1) // 2 + 4, (W - 1) // 2 + 4
    n = F_ * Hs * Ws
    flat = torch.empty(n * 16 + 64, dtype=dtype, device=img.device)
    flat[n * 16:].zero_()
    _check(load().stswin_stem_s2d(_dt(flat), _p(img), _p(flat), F_, H, W, _stream()), "stem_s2d")
    return torch.as_strided(flat, (n, 64), (16, 1)), Hs, Ws


def stem_conv(A, wmat, y, frames, H, W, stats_out=None):
    """y [F*Ho*Wo][64] = the stem convolution of the hip.stem_s2d view A with the packed weights wmat [64][256] (bf16; Wo % 128 == 0)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M = frames * Ho * Wo
    assert A.dtype == torch.bfloat16 and A.stride() == (16, 1) and A.shape[0] == frames * (Ho + 3) * (Wo + 3)
    assert wmat.dtype == torch.bfloat16 and wmat.shape == (64, 256) and wmat.is_contiguous()
    assert y.dtype == torch.bfloat16 and y.shape == (M, 64) and y.is_contiguous()
    assert stats_out is None or (stats_out.dtype == torch.float32 and stats_out.numel() == 2 * 2 * ((M + 255) // 256) * 64)
    with _Span("stem_conv_bf16", 2.0 * M * 64 * 147):
        rc = load().stswin_stem_conv(_p(A), _p(wmat), _p(y), _p(stats_out), frames, H, W, _stream())
    _check(rc, "stem_conv")
    return y


def stem_wgrad_ok(H, W, dtype) -> bool:
    return dtype == torch.bfloat16 and ((W - 1) // 2 + 1) % 128 == 0


def stem_wgrad(dy, A, dw, frames, H, W, accumulate=False):
    """dw fp32 [64][256] (= [cout][tap row][record][16]) from dy [F*Ho*Wo][64] and the hip.stem_s2d view A of the same images."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert dy.dtype == torch.bfloat16 and dy.shape == (frames * Ho * Wo, 64) and dy.is_contiguous()
    assert A.dtype == torch.bfloat16 and A.stride() == (16, 1) and A.shape[0] == frames * (Ho + 3) * (Wo + 3)
    assert dw.dtype == torch.float32 and dw.numel() == 64 * 256 and dw.is_contiguous()
    ws = scratch(dy.device, load().stswin_stem_wgrad_scratch(frames, Ho, Wo))
    with _Span("stem_wgrad_bf16", 2.0 * frames * Ho * Wo * 64 * 147):
        rc = load().stswin_stem_wgrad(_p(dy), _p(A), _p(dw), 1 if accumulate else 0, _p(ws), ws.numel(), frames, H, W, _stream())
    _check(rc, "stem_wgrad")
    return dw


def maxpool3x3s2(src, dst, arg, frames, H, W, Ho, Wo, backward=False):
    """forward: src [F*H*W][C] -> dst [F*Ho*Wo][C] and the winning taps arg (uint8 [F*Ho*Wo][C]); backward: src = d(out), dst = d(in)."""
    C = src.shape[1]
    _pair("maxpool3x3s2", src, dst)
    if (Ho, Wo) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise StswinHipError(f"maxpool3x3s2: ({Ho}, {Wo}) is not the 3x3 stride-2 pad-1 pool of ({H}, {W})")
    _rows("maxpool3x3s2", src, frames * (Ho * Wo if backward else H * W), "src")
    _rows("maxpool3x3s2", dst, frames * (H * W if backward else Ho * Wo), "dst")
    if arg.dtype != torch.uint8 or arg.device != src.device or tuple(arg.shape) != (frames * Ho * Wo, C) or not arg.is_contiguous():
        raise StswinHipError(f"maxpool3x3s2: arg must be a contiguous uint8 [{frames * Ho * Wo}][{C}] on {src.device}, got "
                             f"{arg.dtype} {tuple(arg.shape)} on {arg.device}")
    _check(load().stswin_maxpool3x3s2(_dt(src), _p(src), _ld(src), _p(dst), _ld(dst), _p(arg), frames, H,
                                      W, Ho, Wo, C, 1 if backward else 0, _stream()), "maxpool3x3s2")
    return dst


def conv3x3_c64_ok(frames, H, W, cin, cout, k, stride, pad, dil, dt) -> bool:
    """Geometries stswin_conv3x3_c64 takes (everything else stays on the gather GEMM)."""
    return (dt == torch.bfloat16 and cin == 64 and cout == 64 and k == 3 and stride == 1 and pad == 1 and dil == 1
            and W in (16, 32, 64, 128) and (H * W) % 256 == 0 and frames > 0)


def conv3x3_c64(x, wmat, y, frames, H, W, sign=1, resid=None, stats_out=None):
    """y = conv3x3(x) (sign = +1, wmat = forward matrix) or its input gradient (sign = -1, x = dy, wmat = dgrad matrix)."""
    M = frames * H * W
    for t in (x, y, resid):
        assert t is None or (t.dtype == torch.bfloat16 and t.shape == (M, 64) and t.is_contiguous())
    assert wmat.dtype == torch.bfloat16 and wmat.shape == (64, 576) and wmat.is_contiguous()
    assert stats_out is None or (stats_out.dtype == torch.float32 and stats_out.numel() == 2 * 2 * ((M + 255) // 256) * 64)
    with _Span("conv3x3_c64_bf16", 2.0 * M * 64 * 576):
        rc = load().stswin_conv3x3_c64(_p(x), _p(wmat), _p(y), _p(resid), _p(stats_out), frames, H, W, sign, _stream())
    _check(rc, "conv3x3_c64")
    return y


def conv3x3_c64_wgrad_ok(frames, H, W) -> bool:
    return W in (32, 64, 128) and (H * W) % 128 == 0 and frames > 0


def conv3x3_c64_wgrad(dy, x, dw, frames, H, W, tapminor=True, accumulate=False):
    """dw (fp32, 64*576 values: [64][64][3][3] if tapminor else [64][9][64]) = weight gradient of the 64 -> 64 3x3 convolution."""
    M = frames * H * W
    for t in (dy, x):
        assert t.dtype == torch.bfloat16 and t.shape == (M, 64) and t.is_contiguous()
    assert dw.dtype == torch.float32 and dw.numel() == 64 * 576 and dw.is_contiguous()
    need = load().stswin_conv3x3_c64_wgrad_scratch(frames, H, W)
    ws = scratch(x.device, need)
    with _Span("conv3x3_c64_wgrad_bf16", 2.0 * M * 64 * 576):
        rc = load().stswin_conv3x3_c64_wgrad(_p(dy), _p(x), _p(dw), 1 if tapminor else 0, 1 if accumulate else 0, _p(ws), ws.numel(),
                                             frames, H, W, _stream())
    _check(rc, "conv3x3_c64_wgrad")
    return dw


# ----------------------------------------------------------------------------------------------- GEMMs
def stats_table(M: int, N: int, device) -> torch.Tensor:
    """fp32 [2][2*ceil(M/256)][N] table for gemm_nt(stats_out=...): per-128-row-block column sums | sums of squares."""
    return torch.empty(2, 2 * ((M + 255) // 256), N, dtype=torch.float32, device=device)


def cs_group_reduce(table: torch.Tensor, M: int, groups: int, unit: int = 0):
    """-> (sum, sumsq) fp32 [groups][N] of the statistic groups from a stats_table a gemm_nt filled."""
    N = table.shape[2]
    both = torch.empty(2, groups, N, dtype=torch.float32, device=table.device)
    _check(load().stswin_cs_group_reduce(_p(table), M, N, groups, unit, _p(both[0]), _p(both[1]), _stream()), "cs_group_reduce")
    return both[0], both[1]


def bn_table_finalize(table: torch.Tensor, M: int, running_mean, running_var, groups=1, eps=1e-5, momentum=0.1, unit=0):
    """-> (mean, rstd) fp32 [groups][N] from a stats_table a gemm_nt filled; running statistics updated in place."""
    N = table.shape[2]
    mean = torch.empty(groups, N, dtype=torch.float32, device=table.device)
    rstd = torch.empty_like(mean)
    _check(load().stswin_bn_table_finalize(_p(table), M, N, groups, unit, _p(mean), _p(rstd), _p(running_mean), _p(running_var),
                                           eps, momentum, _stream()), "bn_table_finalize")
    return mean, rstd


def gemm_nt(A: torch.Tensor, Bw: torch.Tensor, out: torch.Tensor, *, M: int, a_rows=None, c_rows=None, bias=None,
            resid=None, r_rows=None, out2=None, S: int = 1, scale: float = 1.0, scale_cols: int = 0, flags: int = 0,
            colsum_out=None, stats_out=None):
    """out[c_rows[m]] = epi(sum_s A[a_rows[s][m], :Kseg] @ Bw[:, s*Kseg:(s+1)*Kseg].T); see include/stswin_hip.h."""
    N, Ktot = Bw.shape
    assert Ktot % S == 0
    Kseg = Ktot // S
    assert A.dtype == Bw.dtype and A.shape[1] >= Kseg
    if not (flags & GF_OUT_F32):
        assert out.dtype == A.dtype
    else:
        assert out.dtype == torch.float32
    cs_table = None
    if stats_out is not None:        # BatchNorm statistics of the output: per-block sums and sums of squares, no reduce here
        assert colsum_out is None and stats_out.shape == (2, 2 * ((M + 255) // 256), N) and stats_out.is_contiguous()
        flags |= GF_CS_PARTIAL | GF_CS_SQ
        colsum_out = stats_out
    elif colsum_out is not None and M >= _CS_PARTIAL_MIN_M and N % 4 == 0 and not (flags & _GF_DEBUG_STAMPS):
        # >= 64 row tiles would each add into the same N addresses: per-block partial sums + one small reduce instead
        cs_table = scratch(A.device, 2 * ((M + 255) // 256) * N)
        flags |= GF_CS_PARTIAL
    elif colsum_out is not None and N % 4 and not _WARNED.get("cs_atomic"):
        _WARNED["cs_atomic"] = True
        import warnings
        warnings.warn(f"stswincl_amd.hip.gemm_nt: column sums of an output with N = {N} (not a multiple of 4) are added with fp32 "
                      f"atomics (order-dependent last bits); pad N to a multiple of 4 for bitwise-reproducible sums")
    name = "gemm_nt_bf16" if A.dtype == torch.bfloat16 else "gemm_nt_f32"
    if _SHAPE_NAMES:
        name += f" M={M} N={N} K={Kseg} S={S} a={int(a_rows is not None)} c={int(c_rows is not None)} fl={flags}"
    # few output tiles, long K (ASPP's dilated convolutions, the 448-channel classifier convolution): ring kernel over tiles x K-splits
    if (_NT_SPLITK and A.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and c_rows is None and resid is None and out2 is None
            and colsum_out is None and scale == 1.0 and scale_cols == 0 and not (flags & ~GF_RELU)):
        need = load().stswin_gemm_nt_splitk_scratch(M, N, Kseg, S)
        if need > 0 and _PLAN_ROWS[0] != 1 and load().stswin_gemm_nt_splitk_scratch(M * _PLAN_ROWS[0], N, Kseg, S) <= 0:
            need = 0
        if need > 0:
            ws = scratch(A.device, need)
            with _Span(name, 2.0 * M * N * Ktot):
                rc = load().stswin_gemm_nt_splitk(_p(A), _ld(A), _p(a_rows), _p(Bw), _ld(Bw), _p(out), _ld(out),
                                                  _p(bias), M, N, Kseg, S, 1 if (flags & GF_RELU) else 0, _p(ws), ws.numel(), _stream())
            if rc != -1008:                  # -1008: not a split-K candidate after all (an `out` column slice that is not 16-byte
                _check(rc, "gemm_nt_splitk")  # aligned, a row pitch that is not a multiple of 8): the tiled kernels below take it
                _log_variant("nt", (M, N, Kseg, S), 0)
                return out
    with _Span(name, 2.0 * M * N * Ktot):
        rc = load().stswin_gemm_nt(
            _dt(A), _p(A), _ld(A), _p(a_rows), _p(Bw), _ld(Bw), _p(out), _ld(out),
            _p(c_rows), _p(out2), _ld(out2) if out2 is not None else 0, _p(bias), _p(resid),
            _ld(resid) if resid is not None else 0, _p(r_rows), M, N, Kseg, S, scale, scale_cols,
            flags, _p(cs_table if cs_table is not None else colsum_out), _stream())
    _check(rc, "gemm_nt")
    _log_variant("nt", (M, N, Kseg, S), 0)
    if cs_table is not None:
        _check(load().stswin_cs_reduce(_p(cs_table), M, N, _p(colsum_out), _stream()), "cs_reduce")
    return out


def gemm_nt_qkv_fp8(A: torch.Tensor, Bw: torch.Tensor, *, M: int, a_rows=None, bias=None, scale: float = 1.0, scale_cols: int = 0,
                    rows_per_problem: int, head_dim: int):
    """QKV projection with an e4m3 result: returns (out8 uint8 [M][N], scales fp32 [M / rows_per_problem][N / head_dim]); see
    include/stswin_hip.h.  Raises StswinHipError on shapes the kernel does not take (the caller keeps the bf16 path for those)."""
    N, K = Bw.shape
    assert A.dtype == torch.bfloat16 and Bw.dtype == torch.bfloat16 and A.shape[1] >= K
    out8 = torch.empty(M, N, dtype=torch.uint8, device=A.device)
    scales = torch.empty(M // rows_per_problem, N // head_dim, dtype=torch.float32, device=A.device)
    with _Span("gemm_nt_bf16" + (f" M={M} N={N} K={K} S=1 a={int(a_rows is not None)} c=0 fl=fp8out" if _SHAPE_NAMES else ""), 2.0 * M * N * K):
        rc = load().stswin_gemm_nt_qkv_fp8(_p(A), _ld(A), _p(a_rows), _p(Bw), _ld(Bw), _p(out8), N, _p(scales),
                                           N // head_dim, _p(bias), M, N, K, scale, scale_cols, rows_per_problem, head_dim,
                                           _stream())
    _check(rc, "gemm_nt_qkv_fp8")
    return out8, scales


VARIANT_LOG = None     # tests: set to a list -> every gemm_nt / gemm_tn / gemm_tn_group launch appends (family, shape, stswin_last_variant)


def _log_variant(family: str, shape, fam_id: int) -> None:
    if VARIANT_LOG is not None:
        VARIANT_LOG.append((family, tuple(int(v) for v in shape), int(load().stswin_last_variant(fam_id))))


_WARNED = {}
# Diagnosis bits of the timeline tools (tools/gemm_timeline.py, tools/attn_qkv_timeline.py), on purpose not in the header: the kernel
# then writes timestamps through one of its output pointers (colsum, qkv_out, dqkv_q_colsum) instead of results
_GF_DEBUG_STAMPS = 1 << 19            # in stswin_gemm_nt's flags
_ATTN_DEBUG_STAMPS = 1 << 30          # in the attention kernels' bias_windows
_NT_SPLITK = os.environ.get("STSWIN_NO_NT_SPLITK") != "1"                 # (A/B switch)
_PLAN_ROWS = [1]             # splitk_as_rows: plan the split-K choice for this many times the launch's rows


class splitk_as_rows:
    """While active, gemm_nt takes its split-K path only where a launch of `factor` times the rows would take it too.  Split-K is
    chosen for few output tiles, so its use depends on the row count, and it adds the K partitions in another order than the tiled
    kernels.  stswincl_amd.video runs the ResNet on one new frame where model(clip) runs it on the clip's four: with factor 4 the
    convolutions of both pick the same kernels, and a frame's features are the same bits in both."""

    def __init__(self, factor: int):
        self.factor = int(factor)

    def __enter__(self):
        self.prev = _PLAN_ROWS[0]
        _PLAN_ROWS[0] = self.factor
        return self

    def __exit__(self, *exc):
        _PLAN_ROWS[0] = self.prev


_CS_PARTIAL_MIN_M = int(os.environ.get("STSWIN_CS_PARTIAL_MIN_M", "1"))   # (the table + fold path is the deterministic one: always)
_TN_WS = {}


def _tn_workspace(device, floats=48 * 1024 * 1024):
    """One scratch buffer per device for the split-K partial slabs (kernels on a stream serialise, so it can be shared)."""
    ws = _TN_WS.get(device)
    if ws is None:
        ws = torch.empty(floats, dtype=torch.float32, device=device)
        _TN_WS[device] = ws
    return ws


_TN_SIDE = {}            # device -> side stream of the deferred combines
_TN_DEFER = 0            # nesting depth of tn_deferred()
_TN_PENDING = None       # event of the last combine launched on the side stream (one at a time: the partials share one workspace)
# OFF by default: measured 0.8-1.0 ms per step SLOWER than the inline combine (536-539 vs 552-556 frames/s, eager and under hipGraph
# replay alike): every cross-stream event edge costs more than the 8 us kernel it hides.  STSWIN_TN_DEFERRED_COMBINE=1 enables it.
_TN_DEFER_ON = os.environ.get("STSWIN_TN_DEFERRED_COMBINE") == "1"


class tn_deferred:
    """with tn_deferred(): the split-K combine of every gemm_tn inside runs on a side stream, ordered behind its GEMM by an event,
    and the calling stream waits for the last one when the block ends - so each combine (5-12 us of a kernel too small to fill
    the chip, plus a launch boundary on either side) overlaps the input-gradient GEMM that follows every weight-gradient GEMM of a
    backward pass.  The next gemm_tn waits for the previous combine before it overwrites the shared partials."""

    def __enter__(self):
        global _TN_DEFER
        _TN_DEFER += 1
        return self

    def __exit__(self, *exc):
        global _TN_DEFER
        _TN_DEFER -= 1
        if _TN_DEFER == 0:
            tn_join()
        return False


def tn_deferred_backward(fn):
    """Decorator for autograd backward functions that issue weight-gradient GEMMs: body inside tn_deferred()."""
    import functools

    @functools.wraps(fn)
    def wrapper(ctx, *grads):
        with tn_deferred():
            return fn(ctx, *grads)
    return wrapper


def tn_join():
    """The current stream waits for the outstanding deferred combine (if any)."""
    global _TN_PENDING
    if _TN_PENDING is not None:
        torch.cuda.current_stream().wait_event(_TN_PENDING)
        _TN_PENDING = None


def gemm_tn(At: torch.Tensor, Bt: torch.Tensor, out_f32: torch.Tensor, *, Mk: int, at_rows=None, bt_rows=None,
            splits: int = 0, bseg: int = 0, atomics: bool = False, overwrite: bool = False, debug_ts: bool = False, tapminor: bool = False):
    """out_f32[i][j] += sum_m At[at_rows[m]][i] * Bt[bt_rows[m]][j]  (fp32); overwrite=True stores instead of adding, so
    out_f32 may come from torch.empty."""
    if overwrite:
        splits |= TN_OVERWRITE
    if tapminor and bseg > 0:            # ask the combine for the [row][channel][tap] order; last_tn_tapminor() says whether it was honoured
        splits |= TN_OUT_TAPMINOR
    Ni, Nj = out_f32.shape
    assert out_f32.dtype == torch.float32 and At.dtype == Bt.dtype
    ws = None if atomics or torch.cuda.is_current_stream_capturing() and At.device not in _TN_WS else _tn_workspace(At.device)
    name = "gemm_tn_bf16" if At.dtype == torch.bfloat16 else "gemm_tn_f32"
    if _SHAPE_NAMES:
        name += f" Mk={Mk} Ni={Ni} Nj={Nj} bseg={bseg} a={int(at_rows is not None)} b={int(bt_rows is not None)}"
    defer = _TN_DEFER > 0 and _TN_DEFER_ON and ws is not None and not debug_ts
    tn_join()                                            # the previous combine still reads the workspace this launch overwrites
    with _Span(name, 2.0 * Mk * Ni * Nj):
        rc = load().stswin_gemm_tn(_dt(At), _p(At), _ld(At), _p(at_rows), _p(Bt), _ld(Bt),
                                   _p(bt_rows), _p(out_f32), (-1 if debug_ts is True else -int(debug_ts)) if debug_ts else _ld(out_f32), Mk, Ni, Nj,
                                   (splits | TN_NO_COMBINE) if defer else splits, bseg, _p(ws),
                                   ws.numel() if ws is not None else 0, _stream())
    _check(rc, "gemm_tn")
    _log_variant("tn", (Mk, Ni, Nj, bseg), 1)
    if defer:
        v = load().stswin_last_variant(1)
        if v & (VAR_TN_SLABS_F32 | VAR_TN_SLABS_BF16):   # partials are waiting in the workspace
            global _TN_PENDING
            cur = torch.cuda.current_stream()
            side = _TN_SIDE.get(At.device)
            if side is None:
                side = _TN_SIDE[At.device] = torch.cuda.Stream(device=At.device)
            ev = torch.cuda.Event()
            ev.record(cur)
            side.wait_event(ev)
            _check(load().stswin_tn_combine(_p(ws), _p(out_f32), _ld(out_f32), Ni, Nj, v >> 16, 1 if (splits & TN_OVERWRITE) else 0,
                                            1 if v & VAR_TN_SLABS_BF16 else 0, side.cuda_stream), "tn_combine")
            _TN_PENDING = torch.cuda.Event()
            _TN_PENDING.record(side)
    return out_f32


class _TnProblem(ctypes.Structure):
    """stswin_tn_problem (include/stswin_hip.h)"""
    _fields_ = [("At", ctypes.c_void_p), ("lda", ctypes.c_long), ("at_rows", ctypes.c_void_p),
                ("Bt", ctypes.c_void_p), ("ldb", ctypes.c_long), ("bt_rows", ctypes.c_void_p),
                ("C", ctypes.c_void_p), ("ldc", ctypes.c_long),
                ("Mk", ctypes.c_int), ("Ni", ctypes.c_int), ("Nj", ctypes.c_int), ("bseg", ctypes.c_int),
                ("overwrite", ctypes.c_int), ("tapminor", ctypes.c_int)]


LAST_TN_GROUP_SPLITS: list = []      # split counts of the last grouped launch (tests, tools)


def gemm_tn_group(problems) -> bool:
    """problems: [dict(At=, Bt=, out=, Mk=, at_rows=None, bt_rows=None, bseg=0, overwrite=True, tapminor=False)] - up to 4 bf16 weight
    gradients of one backward step in ONE launch (stswin_gemm_tn_group).  Returns False when the library declines the set (nothing has
    been written: call gemm_tn for each), True when it was launched."""
    n = len(problems)
    if n == 0:
        return True
    first = problems[0]["At"]
    if n > 4 or first.dtype != torch.bfloat16 or torch.cuda.is_current_stream_capturing() and first.device not in _TN_WS:
        return False
    arr = (_TnProblem * n)()
    flops = 0.0
    for i, q in enumerate(problems):
        At, Bt, out = q["At"], q["Bt"], q["out"]
        assert out.dtype == torch.float32 and At.dtype == Bt.dtype == torch.bfloat16
        ar, br = q.get("at_rows"), q.get("bt_rows")
        arr[i] = _TnProblem(At.data_ptr(), _ld(At), ar.data_ptr() if ar is not None else None, Bt.data_ptr(), _ld(Bt),
                            br.data_ptr() if br is not None else None, out.data_ptr(), _ld(out), q["Mk"], out.shape[0], out.shape[1],
                            q.get("bseg", 0), 1 if q.get("overwrite", True) else 0, 1 if q.get("tapminor", False) else 0)
        flops += 2.0 * q["Mk"] * out.shape[0] * out.shape[1]
    ws = _tn_workspace(first.device)
    tn_join()
    sp = (_c_int * n)()
    name = "gemm_tn_bf16"
    if _SHAPE_NAMES:
        name += " group " + " + ".join(f"{q['out'].shape[0]}x{q['out'].shape[1]}" for q in problems) + f" Mk={problems[0]['Mk']}"
    with _Span(name, flops) as span:
        rc = load().stswin_gemm_tn_group(0, n, arr, _p(ws), ws.numel(), sp, _stream())
        if rc == TN_GROUP_DECLINED:
            span.cancel()
    if rc == TN_GROUP_DECLINED:
        return False
    _check(rc, "gemm_tn_group")
    LAST_TN_GROUP_SPLITS[:] = list(sp)
    _log_variant("tn_group", (n, problems[0]["Mk"]) + tuple(sp), 1)
    return True


def last_tn_tapminor() -> bool:
    """Whether the most recent gemm_tn(tapminor=True) of this thread stored its result tap-minor (it does where split-K slabs are
    combined; a direct-store launch keeps the GEMM order and the caller permutes)."""
    return bool(load().stswin_last_variant(1) & VAR_TN_TAPMINOR)


def last_variant(family: int) -> dict:
    """Which kernel the most recent gemm_nt (family 0) / gemm_tn (family 1) call of this thread launched:
    {kernel, slabs ('' / 'f32' / 'bf16'), splits}.  Test instrumentation (asserts the production dispatch)."""
    v = load().stswin_last_variant(family)
    return {"kernel": v & 0xFFF, "slabs": "bf16" if v & VAR_TN_SLABS_BF16 else ("f32" if v & VAR_TN_SLABS_F32 else ""),
            "splits": v >> 16}


def vec_gather(v: torch.Tensor, imap: torch.Tensor, fill: float = 0.0) -> torch.Tensor:
    """out[i] = v[imap[i]] (fill where imap[i] < 0); v fp32 contiguous, imap int32."""
    out = torch.empty(imap.numel(), dtype=torch.float32, device=v.device)
    _check(load().stswin_vec_gather(_p(v), _p(imap), _p(out), imap.numel(), fill, _stream()), "vec_gather")
    return out


def vec_gather_multi(vs, imap: torch.Tensor, fills=None, outs=None):
    """[out_k[i] = vs[k][imap[i]] (fills[k] where imap[i] < 0)] for up to 4 fp32 contiguous vectors sharing the map, ONE launch.
    outs: write into these tensors (e.g. the running-statistic buffers themselves) instead of fresh ones."""
    k, n = len(vs), imap.numel()
    assert 1 <= k <= 4 and all(v.dtype == torch.float32 and v.is_contiguous() for v in vs)
    if outs is None:
        flat = torch.empty(k, (n + 15) // 16 * 16, dtype=torch.float32, device=imap.device)
        outs = [flat[i, :n] for i in range(k)]
    else:
        assert len(outs) == k and all(o.dtype == torch.float32 and o.is_contiguous() and o.numel() == n for o in outs)
    fills = list(fills) if fills is not None else [0.0] * k
    _check(load().stswin_vec_gather_multi(k, (_c_void_p * k)(*[v.data_ptr() for v in vs]), _p(imap), (_c_void_p * k)(*[o.data_ptr() for o in outs]),
                                          n, (_c_float * k)(*[float(f) for f in fills]), _stream()), "vec_gather_multi")
    return outs


def colsum(y: torch.Tensor, out_f32: torch.Tensor, M: Optional[int] = None):
    M = y.shape[0] if M is None else M
    lib = load()
    ws = scratch(y.device, lib.stswin_colsum_scratch(M, y.shape[1]))
    _check(lib.stswin_colsum(_dt(y), _p(y), _ld(y), _p(out_f32), M, y.shape[1], _p(ws), _stream()), "colsum")
    return out_f32


# ----------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, *, M, rows=None, S=1, Cseg=None, eps=1e-5, save_stats=True, out=None):
    Cseg = x.shape[1] if Cseg is None else Cseg
    if out is not None:                       # caller-provided destination (a row block of a larger buffer)
        assert out.shape == (M, S * Cseg) and out.dtype == x.dtype and out.stride(1) == 1
        y = out
    else:
        y = torch.empty(M, S * Cseg, dtype=x.dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    rc = load().stswin_layernorm_fwd(_dt(x), _p(x), _ld(x), _p(rows), S, Cseg, _p(y), _ld(y),
                                     _p(gamma), _p(beta), _p(mean), _p(rstd), M, eps, _stream())
    _check(rc, "layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, *, M, rows=None, S=1, Cseg=None, dx=None, accumulate=False,
                  dxsum=None, add=None):
    """add (optional): dx = add + LN'(dy) into a fresh (or the given) dx, `add` left intact."""
    Cseg = x.shape[1] if Cseg is None else Cseg
    if dx is None:
        dx = torch.empty_like(x)
        accumulate = False
    ws = scratch(x.device, load().stswin_layernorm_bwd_scratch(M, S * Cseg))
    if add is not None:
        assert not accumulate and add.dtype == x.dtype
        rc = load().stswin_layernorm_bwd_add(_dt(x), _p(dy), _ld(dy), _p(x), _ld(x), _p(rows), S, Cseg,
                                             _p(gamma), _p(mean), _p(rstd), _p(add), _ld(add), _p(dx), _ld(dx),
                                             _p(dgamma), _p(dbeta), M, _p(dxsum), _p(ws), _stream())
        _check(rc, "layernorm_bwd_add")
        return dx
    rc = load().stswin_layernorm_bwd(_dt(x), _p(dy), _ld(dy), _p(x), _ld(x), _p(rows), S, Cseg,
                                     _p(gamma), _p(mean), _p(rstd), _p(dx), _ld(dx), _p(dgamma), _p(dbeta), M,
                                     1 if accumulate else 0, _p(dxsum), _p(ws), _stream())
    _check(rc, "layernorm_bwd")
    return dx


# ----------------------------------------------------------------------------------------------- attention
def bias_expand(table, index, mask, N, heads):
    """relative_position_bias_table[index] as [heads][key][query] fp32, or [nW][heads][key][query] with the mask added."""
    nW = mask.shape[0] if mask is not None else 1
    out = torch.empty((nW, heads, N, N) if mask is not None else (heads, N, N), dtype=torch.float32, device=table.device)
    assert table.dtype == torch.float32 and table.is_contiguous() and index.dtype == torch.int64 and index.is_contiguous()
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous())
    _check(load().stswin_bias_expand(_p(table), _p(index), _p(mask), _p(out), N, heads, nW, _stream()), "bias_expand")
    return out


def bias_expand_multi(entries) -> None:
    """entries: [(table, index, mask or None, out, N, heads)] - bias_expand of every entry into its existing `out`, 16 per launch."""
    lib, st = load(), _stream()
    for lo in range(0, len(entries), 16):
        ch = entries[lo:lo + 16]
        k = len(ch)
        arr = lambda i: (_c_void_p * k)(*[(e[i].data_ptr() if e[i] is not None else 0) for e in ch])   # noqa: E731
        _check(lib.stswin_bias_expand_multi(k, arr(0), arr(1), arr(2), arr(3), (_c_int * k)(*[e[4] for e in ch]), (_c_int * k)(*[e[5] for e in ch]),
                                            (_c_int * k)(*[(e[2].shape[0] if e[2] is not None else 1) for e in ch]), st), "bias_expand_multi")


def scatter_lists(index: torch.Tensor, table_rows: int):
    """(order, offs) of stswin_bias_scatter for an index buffer: the pairs i * N + j sorted (stably) by their table row and the start of
    every row's range.  Three small torch kernels, no host sync; callers that scatter through the same index every step keep the
    result (ops.py caches it per window size: relative_position_index is a function of the window size alone)."""
    flat = index.reshape(-1)
    order = torch.argsort(flat, stable=True).to(torch.int32).contiguous()
    counts = torch.bincount(flat, minlength=table_rows)[:table_rows]
    offs = torch.zeros(table_rows + 1, dtype=torch.int32, device=index.device)
    offs[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return order, offs.contiguous()


def bias_scatter(dbiasT, index, dtable, N, heads, lists=None):
    assert dbiasT.is_contiguous() and dtable.is_contiguous() and index.dtype == torch.int64 and index.is_contiguous()
    assert dtable.shape[0] * dtable.shape[1] == dtable.numel() and dtable.shape[1] == heads
    order, offs = lists if lists is not None else scatter_lists(index, dtable.shape[0])
    _check(load().stswin_bias_scatter(_p(dbiasT), _p(order), _p(offs), _p(dtable), N, heads, dtable.shape[0], 1, _stream()), "bias_scatter")
    return dtable


def _bias_windows(biasT, maskT, nW, bias_index=None):
    """biasT [heads][N][N] (+ optional maskT) or the pre-summed per-window table [nW][heads][N][N] (maskT None)."""
    if biasT.dim() == 4:
        assert maskT is None and (biasT.shape[0] == nW or bias_index is not None)
        return biasT.shape[0]
    return 1


def win_attn_fwd(qkv, biasT, maskT, *, nB_, nW, T, ws, heads, C, bias_index=None, fp8=False):
    out = torch.empty(qkv.shape[0], C, dtype=qkv.dtype, device=qkv.device)
    if fp8:
        if qkv.dtype != torch.bfloat16:
            raise StswinHipError("fp8 attention quantises bf16 q / k / v")
        rc = load().stswin_win_attn_fwd_fp8(_p(qkv), _ld(qkv), _p(out), _ld(out), _p(biasT), _p(maskT), nB_, nW, T, ws,
                                            heads, C, _bias_windows(biasT, maskT, nW, bias_index), _p(bias_index), _stream())
        _check(rc, "win_attn_fwd_fp8")
        return out
    rc = load().stswin_win_attn_fwd(_dt(qkv), _p(qkv), _ld(qkv), _p(out), _ld(out), _p(biasT),
                                    _p(maskT), nB_, nW, T, ws, heads, C, _bias_windows(biasT, maskT, nW, bias_index), _p(bias_index),
                                    _stream())
    _check(rc, "win_attn_fwd")
    return out


def win_attn_fwd_f8(qkv8, scales, biasT, maskT, *, nB_, nW, T, ws, heads, C, bias_index=None):
    """Attention forward on e4m3-stored q | k | v (gemm_nt_qkv_fp8): bf16 [rows][C]."""
    assert qkv8.dtype == torch.uint8 and qkv8.is_contiguous() and scales.dtype == torch.float32 and scales.is_contiguous()
    out = torch.empty(qkv8.shape[0], C, dtype=torch.bfloat16, device=qkv8.device)
    with _Span("attn_fwd_f8", 4.0 * nB_ * heads * (T * ws * ws) ** 2 * (C // heads)):
        rc = load().stswin_win_attn_fwd_f8(_p(qkv8), qkv8.shape[1], _p(scales), scales.shape[1], _p(out), _ld(out),
                                           _p(biasT), _p(maskT), nB_, nW, T, ws, heads, C, _bias_windows(biasT, maskT, nW, bias_index),
                                           _p(bias_index), _stream())
    _check(rc, "win_attn_fwd_f8")
    return out


def win_attn_bwd_f8(qkv8, scales, dout, biasT, maskT, dbiasT, *, nB_, nW, T, ws, heads, C, scale, colsum_out=None, bias_index=None):
    """Attention backward on e4m3-stored q | k | v: bf16 dqkv [rows][3C]."""
    dqkv = torch.empty(qkv8.shape[0], 3 * C, dtype=torch.bfloat16, device=qkv8.device)
    lib = load()
    need = lib.stswin_win_attn_bwd_scratch(nB_, ws, heads, C)
    if need < 0:
        raise StswinHipError(f"win_attn_bwd_f8: bad geometry ({need})")
    sc = scratch(qkv8.device, need)
    with _Span("attn_bwd_f8", 10.0 * nB_ * heads * (T * ws * ws) ** 2 * (C // heads)):
        rc = lib.stswin_win_attn_bwd_f8(_p(qkv8), qkv8.shape[1], _p(scales), scales.shape[1], _p(dout), _ld(dout),
                                        _p(dqkv), _ld(dqkv), _p(biasT), _p(maskT), _p(dbiasT), _p(colsum_out), nB_, nW, T, ws, heads, C,
                                        scale, _bias_windows(biasT, maskT, nW, bias_index), _p(bias_index), _p(sc),
                                        sc.numel(), _stream())
    _check(rc, "win_attn_bwd_f8")
    return dqkv


def win_attn_qkv_fwd(x, rmap, w, bqkv, biasT, *, nB_, nW, T, ws, heads, C, scale, bias_index=None, want_qkv=True, debug_ts=None):
    """QKV-fused window attention forward (include/stswin_hip.h: stswin_win_attn_qkv_fwd) -> (out [nB_*T*ws*ws][C], qkv or None)."""
    rows = nB_ * T * ws * ws
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise StswinHipError("win_attn_qkv_fwd is a bf16 kernel")
    out = torch.empty(rows, C, dtype=x.dtype, device=x.device)
    qkv = torch.empty(rows, 3 * C, dtype=x.dtype, device=x.device) if want_qkv else None
    if debug_ts is not None:                     # tools/attn_qkv_timeline.py: int64 [256][8][8] stamp buffer in place of qkv_out
        rc = load().stswin_win_attn_qkv_fwd(_p(x), _ld(x), x.shape[0], _p(rmap), _p(w), _ld(w), _p(bqkv), _p(debug_ts), 0,
                                            _p(out), _ld(out), _p(biasT), nB_, nW, T, ws, heads, C, scale,
                                            _bias_windows(biasT, None, nW, bias_index) | _ATTN_DEBUG_STAMPS, _p(bias_index), _stream())
        _check(rc, "win_attn_qkv_fwd")
        return out, None
    name = "attn_qkv_fwd_bf16"
    with _Span(name, 2.0 * rows * 3 * C * C + 4.0 * nB_ * heads * (T * ws * ws) ** 2 * (C // heads)):
        rc = load().stswin_win_attn_qkv_fwd(_p(x), _ld(x), x.shape[0], _p(rmap), _p(w), _ld(w), _p(bqkv), _p(qkv),
                                            _ld(qkv) if qkv is not None else 0, _p(out), _ld(out), _p(biasT), nB_, nW, T,
                                            ws, heads, C, scale, _bias_windows(biasT, None, nW, bias_index), _p(bias_index),
                                            _stream())
    _check(rc, "win_attn_qkv_fwd")
    return out, qkv


def win_attn_qkv_fwd_ok(x: torch.Tensor) -> bool:
    """Whether the fused kernel's 32-bit buffer offsets reach every token row of x (stswin_win_attn_qkv_fwd returns -1208 otherwise)."""
    return x.shape[0] * _ld(x) * 2 <= 0xFFFF0000


def win_attn_bwd(qkv, dout, biasT, maskT, dbiasT, *, nB_, nW, T, ws, heads, C, scale, colsum_out=None, debug_ts=False,
                 bias_index=None):
    dqkv = torch.empty_like(qkv)
    lib = load()
    need = lib.stswin_win_attn_bwd_scratch(nB_, ws, heads, C)
    if need < 0:
        raise StswinHipError(f"win_attn_bwd: bad geometry ({need})")
    sc = scratch(qkv.device, need)
    rc = load().stswin_win_attn_bwd(_dt(qkv), _p(qkv), _ld(qkv), _p(dout), _ld(dout), _p(dqkv),
                                    _ld(dqkv), _p(biasT), _p(maskT), _p(dbiasT), _p(colsum_out), nB_, nW, T, ws, heads, C,
                                    scale, _bias_windows(biasT, maskT, nW, bias_index) | (_ATTN_DEBUG_STAMPS if debug_ts else 0),
                                    _p(bias_index), _p(sc), sc.numel(), _stream())
    _check(rc, "win_attn_bwd")
    return dqkv


# ----------------------------------------------------------------------------------------------- head ops
def colstats(x, groups=1, squares=True, M=None, unit=0):
    M = x.shape[0] if M is None else M
    C = x.shape[1]
    both = zeros(2 if squares else 1, groups, C, device=x.device)
    s = both[0]
    ss = both[1] if squares else None
    lib = load()
    need = lib.stswin_colstats_scratch(_dt(x), M, C, groups, unit)
    if need < 0:
        raise StswinHipError(f"colstats: bad geometry ({need})")
    _check(lib.stswin_colstats(_dt(x), _p(x), _ld(x), _p(s), _p(ss), M, C, groups, unit, _p(scratch(x.device, need)), _stream()),
           "colstats")
    return s, ss


def bn_finalize(x, s, ss, running_mean, running_var, groups=1, eps=1e-5, momentum=0.1, M=None, unit=0, raw=False):
    """raw=True: s / ss are plain sums (from a GEMM epilogue, hip.cs_group_reduce), not pivot-shifted ones (hip.colstats)."""
    M = x.shape[0] if M is None else M
    C = x.shape[1]
    mean = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(groups, C, dtype=torch.float32, device=x.device)
    _check(load().stswin_bn_finalize(_dt(x), _p(None if raw else x), _ld(x), _p(s), _p(ss), _p(mean), _p(rstd), _p(running_mean),
                                     _p(running_var), M, C, groups, eps, momentum, unit, _stream()),
           "bn_finalize")
    return mean, rstd


def bn_apply(x, mean, rstd, gamma, beta, out, resid=None, groups=1, relu=True, M=None, unit=0):
    M = x.shape[0] if M is None else M
    _check(load().stswin_bn_apply(_dt(x), _p(x), _ld(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(resid),
                                  _ld(resid) if resid is not None else 0, _p(out), _ld(out), M,
                                  x.shape[1], groups, 1 if relu else 0, unit, _stream()), "bn_apply")
    return out


def bn_bwd(dy, x, y, mean, rstd, gamma, dx, dresid=None, groups=1, relu=True, training=True, M=None, phase=0, sums=None,
           rows_total=0, beta=None, unit=0, group_sums=None):
    M = x.shape[0] if M is None else M
    C = x.shape[1]
    if sums is None:
        both = zeros(2, groups, C, device=x.device)
        s1, s2 = both[0], both[1]
    else:
        s1, s2 = sums
    lib = load()
    need = lib.stswin_bn_bwd_scratch(_dt(x), M, C, groups, unit) if phase != 2 else 0
    if need < 0:
        raise StswinHipError(f"bn_bwd: bad geometry ({need})")
    _check(lib.stswin_bn_bwd(_dt(x), _p(dy), _ld(dy), _p(x), _ld(x), _p(y),
                                _ld(y) if y is not None else 0, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(s1), _p(s2),
                                _p(dx), _ld(dx), _p(dresid), _ld(dresid) if dresid is not None else 0, M, C,
                                groups, 1 if relu else 0, 1 if training else 0, phase, rows_total, unit, _p(group_sums),
                                _p(scratch(x.device, need) if phase != 2 else None), _stream()), "bn_bwd")
    return s1, s2


def bn_relu_pool(x, mean, rstd, gamma, beta, frames, H, W, groups=1, unit=0):
    """-> (pooled [frames*Hp*Wp][C], arg uint8): BatchNorm + ReLU + MaxPool2d(3, 2, 1) of x [frames*H*W][C] in one pass."""
    C = x.shape[1]
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty(frames * Hp * Wp, C, dtype=x.dtype, device=x.device)
    arg = torch.empty(frames * Hp * Wp, C, dtype=torch.uint8, device=x.device)
    _check(load().stswin_bn_relu_pool(_dt(x), _p(x), _ld(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(out), _ld(out),
                                      _p(arg), frames, H, W, C, groups, unit, _stream()), "bn_relu_pool")
    return out, arg


def _pair(fn: str, src: torch.Tensor, dst: torch.Tensor) -> None:
    """Source and destination of a token kernel: one dtype (the kernel is instantiated for ONE element type and reads both through
    it), one device, one width.  Raises before anything is launched."""
    if src.dtype != dst.dtype:
        raise StswinHipError(f"{fn}: source is {src.dtype} but destination is {dst.dtype}")
    if src.device != dst.device:
        raise StswinHipError(f"{fn}: source on {src.device} but destination on {dst.device}")
    if src.dim() != 2 or dst.dim() != 2 or src.shape[1] != dst.shape[1]:
        raise StswinHipError(f"{fn}: source {tuple(src.shape)} and destination {tuple(dst.shape)} must be 2-D and equally wide")


def _rows(fn: str, t: torch.Tensor, rows: int, what: str) -> None:
    if t.shape[0] != rows:
        raise StswinHipError(f"{fn}: {what} has {t.shape[0]} rows, the stated geometry needs {rows}")


def rows_broadcast(v, out, groups, scale=1.0, accumulate=False, M=None):
    """out[r] (+)= v[r // (M / groups)] * scale for the first M rows of out: v fp32 [groups][C], contiguous."""
    M = out.shape[0] if M is None else M
    if v.dtype != torch.float32 or not v.is_contiguous():
        raise StswinHipError(f"rows_broadcast: v must be a contiguous fp32 matrix, got {v.dtype}, strides {tuple(v.stride())}")
    if v.device != out.device:
        raise StswinHipError(f"rows_broadcast: v on {v.device} but out on {out.device}")
    if v.dim() != 2 or out.dim() != 2 or v.shape[1] != out.shape[1]:
        raise StswinHipError(f"rows_broadcast: v {tuple(v.shape)} and out {tuple(out.shape)} must be 2-D and equally wide")
    if groups <= 0 or v.shape[0] != groups or M > out.shape[0] or M % groups:
        raise StswinHipError(f"rows_broadcast: v has {v.shape[0]} rows for {groups} groups; M = {M} of out's {out.shape[0]} rows")
    _check(load().stswin_rows_broadcast(_dt(out), _p(v), _p(out), _ld(out), M, v.shape[1], groups,
                                        scale, 1 if accumulate else 0, _stream()), "rows_broadcast")
    return out


def bilinear(src, dst, frames, h, w, H, W, backward=False):
    """forward: src [F*h*w][C] -> dst [F*H*W][C]; backward: src = d(out) [F*H*W][C] -> dst = d(in) [F*h*w][C]."""
    C = dst.shape[1]
    _pair("bilinear", src, dst)
    _rows("bilinear", src, frames * (H * W if backward else h * w), "src")
    _rows("bilinear", dst, frames * (h * w if backward else H * W), "dst")
    _check(load().stswin_bilinear(_dt(src), _p(src), _ld(src), _p(dst), _ld(dst), frames, h, w, H, W, C,
                                  1 if backward else 0, _stream()), "bilinear")
    return dst


def logits_upsample(tokens, nchw, frames, h, w, H, W, nc, backward=False):
    """forward: tokens [F*h*w][>= nc] -> nchw [F][nc][H][W]; backward: nchw = d(logits) -> columns < nc of tokens = d(tokens)."""
    if tokens.dtype != nchw.dtype:
        raise StswinHipError(f"logits_upsample: tokens are {tokens.dtype} but the NCHW tensor is {nchw.dtype}")
    if tokens.device != nchw.device:
        raise StswinHipError(f"logits_upsample: tokens on {tokens.device} but the NCHW tensor on {nchw.device}")
    if tokens.dim() != 2 or tokens.shape[1] < nc or nc <= 0:
        raise StswinHipError(f"logits_upsample: tokens {tuple(tokens.shape)} cannot hold {nc} classes")
    _rows("logits_upsample", tokens, frames * h * w, "tokens")
    if nchw.numel() != frames * nc * H * W or not nchw.is_contiguous():
        raise StswinHipError(f"logits_upsample: the NCHW tensor {tuple(nchw.shape)} is not a contiguous [{frames}][{nc}][{H}][{W}]")
    _check(load().stswin_logits_upsample(_dt(tokens), _p(tokens), _ld(tokens), _p(nchw), frames, h, w, H, W, nc,
                                         1 if backward else 0, _stream()), "logits_upsample")


def ce_fwd(logits, labels, ignore_index, thresh):
    F_, nc = logits.shape[:2]
    HW = logits[0, 0].numel()
    loss = torch.empty(F_ * HW, dtype=torch.float32, device=logits.device)
    stats = zeros(4, device=logits.device)          # [count, #labels outside [0, nc), 64-bit fixed-point sum]: include/stswin_hip.h
    _check(load().stswin_ce_fwd(_dt(logits), _p(logits), _p(labels), _p(loss), _p(stats), F_, HW, nc, ignore_index,
                                thresh, _stream()), "ce_fwd")
    return loss, stats


def ohem_select(loss, stats, n_min: int, thresh: float):
    """(value [1], sel [4]) of OhemCELoss2D's selection (losses.py:35-39) on the device: no sort, no host sync.
    sel = (cut, weight above the cut, top-n_min branch taken, weight at the cut): include/stswin_hip.h."""
    work = torch.empty(OHEM_WORK_BYTES // 4, dtype=torch.int32, device=loss.device)
    value = torch.empty((), dtype=torch.float32, device=loss.device)
    sel = torch.empty(4, dtype=torch.float32, device=loss.device)
    _check(load().stswin_ohem_select(_p(loss), loss.numel(), n_min, thresh, _p(stats), _p(work),
                                     OHEM_WORK_BYTES, _p(value), _p(sel), _stream()), "ohem_select")
    return value, sel


def ce_bwd(logits, labels, loss, sel, gscale, ignore_index):
    F_, nc = logits.shape[:2]
    HW = logits[0, 0].numel()
    d = torch.empty_like(logits)
    _check(load().stswin_ce_bwd(_dt(logits), _p(logits), _p(labels), _p(loss), _p(sel), _p(gscale), _p(d), F_, HW,
                                nc, ignore_index, _stream()), "ce_bwd")
    return d


def contrast_fwd(q, keys, lq, lks, N, HW):
    """q [N*HW][C], keys 5 x [N*HW][C] (same pitch), lq / lks int32 [N][HW] -> pos, all fp32 [N][HW][5]."""
    C = q.shape[1]
    assert len(keys) == 5 and len(lks) == 5 and all(k.dtype == q.dtype and _ld(k) == _ld(keys[0]) for k in keys)
    pos = torch.empty(N, HW, 5, dtype=torch.float32, device=q.device)
    tot = torch.empty(N, HW, 5, dtype=torch.float32, device=q.device)
    K5 = (_c_void_p * 5)(*[k.data_ptr() for k in keys])
    L5 = (_c_void_p * 5)(*[l.data_ptr() for l in lks])
    with _Span("contrast_fwd_bf16" if q.dtype == torch.bfloat16 else "contrast_fwd_f32", 2.0 * N * HW * 5 * HW * C):
        rc = load().stswin_contrast_fwd(_dt(q), _p(q), _ld(q), K5, _ld(keys[0]), _p(lq), L5, _p(pos),
                                        _p(tot), N, HW, C, _stream())
    _check(rc, "contrast_fwd")
    return pos, tot


_BANK_WS = {}


def _bank_workspace(device, floats):
    ws = _BANK_WS.get(device)
    if ws is None or ws.numel() < floats:
        ws = torch.empty(max(floats, 1 << 22), dtype=torch.float32, device=device)
        _BANK_WS[device] = ws
    return ws


def contrast_bank_fwd(Q, lq, bank, lb, *, q_sets, q_block, bank_block, gmap, inv_tau=1.0, want_lse=False, unit_rows=False):
    """Q [M][C], lq int32 [M]; bank [maps][seg][C], lb int32 [maps][seg]; gmap: q_sets lists of map indices (one per group).
    -> pos, all fp32 [M][groups] (+ rowmax, lse fp32 [M] or None, None); see include/stswin_hip.h."""
    M, C = Q.shape
    maps, seg = bank.shape[0], bank.shape[1]
    groups = len(gmap[0])
    assert Q.dtype == bank.dtype and bank.is_contiguous() and lb.is_contiguous() and lq.is_contiguous()
    assert lq.dtype == torch.int32 and lb.dtype == torch.int32 and len(gmap) == q_sets and all(len(g) == groups for g in gmap)
    if lq.numel() != M or lb.shape != (maps, seg):
        raise StswinHipError(f"contrast_bank_fwd: {lq.numel()} query labels for {M} query rows, bank labels {tuple(lb.shape)} for a "
                             f"{maps} x {seg} bank")
    pos = torch.empty(M, groups, dtype=torch.float32, device=Q.device)
    tot = torch.empty(M, groups, dtype=torch.float32, device=Q.device)
    rowmax = torch.empty(M, dtype=torch.float32, device=Q.device) if want_lse else None
    lse = torch.empty(M, dtype=torch.float32, device=Q.device) if want_lse else None
    ws = _bank_workspace(Q.device, 4 * M * groups * 8)
    gm = (_c_int * (q_sets * groups))(*[int(v) for row in gmap for v in row])
    name = "contrast_bank_fwd_bf16" if Q.dtype == torch.bfloat16 else "contrast_bank_fwd_f32"
    fn = load().stswin_contrast_bank_fwd_unit if unit_rows else load().stswin_contrast_bank_fwd     # unit_rows: L2-normalised Q / bank rows
    with _Span(name, 2.0 * M * groups * bank_block * C):
        rc = fn(_dt(Q), _p(Q), _ld(Q), _p(lq), M, C, q_sets, q_block, _p(bank),
                                             bank.stride(1), _p(lb), maps, seg, bank_block, groups, gm, inv_tau,
                                             _p(pos), _p(tot), _p(rowmax), _p(lse), _p(ws), ws.numel(), _stream())
    _check(rc, "contrast_bank_fwd")
    return pos, tot, rowmax, lse


def contrast_class_sums(bank, lb, bank_block, ncls):
    """-> ksum fp32 [maps][seg / bank_block][ncls + 1][C]: per-class sums of the bank rows (slot ncls: all rows)."""
    maps, seg, C = bank.shape
    ksum = torch.empty(maps, seg // bank_block, ncls + 1, C, dtype=torch.float32, device=bank.device)
    lib = load()
    need = lib.stswin_contrast_class_sums_scratch(maps, seg, bank_block, C, ncls)
    if need < 0:
        raise StswinHipError(f"contrast_class_sums: bad geometry ({need})")
    _check(lib.stswin_contrast_class_sums(_dt(bank), _p(bank), bank.stride(1), _p(lb), maps, seg, bank_block, C, ncls,
                                          _p(ksum), _p(scratch(bank.device, need)), _stream()), "contrast_class_sums")
    return ksum


def contrast_bank_dq(dpos, dneg, cnt, lq, ksum, *, q_sets, q_block, seg, bank_block, gmap):
    M, groups = dpos.shape
    C, ncls = ksum.shape[3], ksum.shape[2] - 1
    dq = torch.empty(M, C, dtype=torch.float32, device=dpos.device)
    gm = (_c_int * (q_sets * groups))(*[int(v) for row in gmap for v in row])
    _check(load().stswin_contrast_bank_dq(_p(dpos.contiguous()), _p(dneg.contiguous()), _p(cnt.contiguous()), _p(lq), _p(ksum), _p(dq), C, M, C,
                                          q_sets, q_block, seg, bank_block, ncls, groups, gm, _stream()), "contrast_bank_dq")
    return dq


def rownorm_scatter(X: torch.Tensor, Y: torch.Tensor, views: int, HW: int, samples: int, want_inv: bool = False):
    """Y[view][sample * HW + px] = normalize(X[(sample * views + view) * HW + px]) (fp32 arithmetic, Y's dtype = X's); -> inv or None."""
    R, C = X.shape
    assert Y.dtype == X.dtype and Y.shape == (R, C) and X.stride(1) == 1 and Y.stride(1) == 1
    inv = torch.empty(R, dtype=torch.float32, device=X.device) if want_inv else None
    _check(load().stswin_rownorm_scatter(_dt(X), _p(X), X.stride(0), _p(Y), Y.stride(0), _p(inv), R, C, views, HW, samples,
                                         _stream()), "rownorm_scatter")
    return inv


def rownorm_scatter_bwd(X: torch.Tensor, inv: torch.Tensor, dY: torch.Tensor, views: int, HW: int, samples: int) -> torch.Tensor:
    R, C = X.shape
    assert dY.dtype == torch.float32 and dY.shape == (R, C) and dY.stride(1) == 1
    dX = torch.empty(R, C, dtype=X.dtype, device=X.device)
    _check(load().stswin_rownorm_scatter_bwd(_dt(X), _p(X), X.stride(0), _p(inv), _p(dY), dY.stride(0), _p(dX), C, R, C,
                                             views, HW, samples, _stream()), "rownorm_scatter_bwd")
    return dX


def labels_resize(masks, h: int, w: int) -> torch.Tensor:
    """len(masks) float label maps (N, 1, Hs, Ws) -> int32 [maps][N * h * w] (nearest neighbour + truncation)."""
    N, _, Hs, Ws = masks[0].shape
    ms = [m.contiguous() if (m.dtype == torch.float32 and m.is_contiguous()) else m.float().contiguous() for m in masks]
    assert all(m.shape == (N, 1, Hs, Ws) and m.is_cuda for m in ms)
    lb = torch.empty(len(ms), N * h * w, dtype=torch.int32, device=ms[0].device)
    arr = (_c_void_p * len(ms))(*[m.data_ptr() for m in ms])
    _check(load().stswin_labels_resize(arr, len(ms), N, Hs, Ws, h, w, _p(lb), _stream()), "labels_resize")
    return lb


def label_counts(lq: torch.Tensor, lb: torch.Tensor, *, q_sets, q_block, bank_block, ncls, gmap) -> torch.Tensor:
    """cnt fp32 [M][groups]: visible bank rows of each group whose label equals the query's."""
    M, (maps, seg), groups = lq.numel(), lb.shape, len(gmap[0])
    if M % q_sets or (M // q_sets) % q_block or seg % bank_block or not lq.is_contiguous() or not lb.is_contiguous():
        raise StswinHipError(f"label_counts: {M} query labels do not split into {q_sets} sets of {q_block}-row blocks "
                             f"(bank {maps} x {seg}, blocks of {bank_block})")
    hist = torch.empty(maps, seg // bank_block, ncls, dtype=torch.int32, device=lq.device)
    cnt = torch.empty(M, groups, dtype=torch.float32, device=lq.device)
    gm = (_c_int * (q_sets * groups))(*[int(v) for row in gmap for v in row])
    _check(load().stswin_label_counts(_p(lq), _p(lb), M, maps, seg, q_sets, q_block, bank_block, ncls, groups, gm, _p(hist), _p(cnt), _stream()),
           "label_counts")
    return cnt


def pair_loss(pos, tot, cnt, q_sets: int, visible: int) -> torch.Tensor:
    M, groups = pos.shape
    loss = torch.empty(1, dtype=torch.float32, device=pos.device)
    _check(load().stswin_pair_loss(_p(pos), _p(tot), _p(cnt), M, groups, q_sets, visible, _p(loss), _stream()), "pair_loss")
    return loss


def pair_loss_bwd(pos, tot, cnt, dloss, q_sets: int, visible: int):
    M, groups = pos.shape
    dpos, dneg = torch.empty_like(pos), torch.empty_like(pos)
    _check(load().stswin_pair_loss_bwd(_p(pos), _p(tot), _p(cnt), _p(dloss), M, groups, q_sets, visible, _p(dpos), _p(dneg), _stream()),
           "pair_loss_bwd")
    return dpos, dneg


def upsample_argmax(logits, H, W, gt=None):
    """NCHW logits [F][nc][h][w] -> uint8 labels [F][H][W] (+ int32 counts [F][3][nc] when gt int64 [F][H][W] is given)."""
    F_, nc, h, w = logits.shape
    lg = logits.contiguous()
    labels = torch.empty(F_, H, W, dtype=torch.uint8, device=logits.device)
    counts = torch.zeros(F_, 3, nc, dtype=torch.int32, device=logits.device) if gt is not None else None
    _check(load().stswin_upsample_argmax(_dt(lg), _p(lg), _p(labels), _p(gt.contiguous() if gt is not None else None),
                                         _p(counts), F_, nc, h, w, H, W, _stream()), "upsample_argmax")
    return labels, counts


def upsample_argmax_cm(logits, H, W, gt=None, cm=None, align_corners=True, labels=True):
    """NCHW logits [F][nc][h][w] (bf16 / fp32, nc <= 64) -> uint8 labels [F][H][W] of the bilinear resize (align_corners as
    F.interpolate) + argmax, or None with labels=False.  With gt (int64 [F][H][W]) and cm (int64 [ncm][ncm] on the device) every
    pixel with gt and label in [0, ncm) adds 1 to cm[gt][label]; cm is accumulated, not cleared (include/stswin_hip.h,
    stswin_upsample_argmax_cm)."""
    if logits.dim() != 4:
        raise StswinHipError(f"upsample_argmax_cm: logits must be [F][nc][h][w], got {tuple(logits.shape)}")
    F_, nc, h, w = logits.shape
    if not 1 <= nc <= 64:
        raise StswinHipError(f"upsample_argmax_cm: {nc} classes, the kernel takes 1 .. 64")
    if (gt is None) != (cm is None):
        raise StswinHipError("upsample_argmax_cm: gt and cm go together")
    if gt is None and not labels:
        raise StswinHipError("upsample_argmax_cm: neither labels nor a confusion matrix asked for")
    ncm = 0
    if gt is not None:
        if gt.dtype != torch.int64 or tuple(gt.shape) != (F_, H, W) or gt.device != logits.device:
            raise StswinHipError(f"upsample_argmax_cm: gt must be int64 [{F_}][{H}][{W}] on {logits.device}, got {gt.dtype} "
                                 f"{tuple(gt.shape)} on {gt.device}")
        if cm.dtype != torch.int64 or cm.dim() != 2 or cm.shape[0] != cm.shape[1] or not cm.is_contiguous() or cm.device != logits.device:
            raise StswinHipError(f"upsample_argmax_cm: cm must be contiguous int64 [ncm][ncm] on {logits.device}, got {cm.dtype} "
                                 f"{tuple(cm.shape)}")
        ncm = cm.shape[0]
        if not 1 <= ncm <= 64:
            raise StswinHipError(f"upsample_argmax_cm: a {ncm} x {ncm} matrix, the kernel takes 1 .. 64 classes")
        gt = gt.contiguous()
    lg = logits.contiguous()
    out = torch.empty(F_, H, W, dtype=torch.uint8, device=logits.device) if labels else None
    _check(load().stswin_upsample_argmax_cm(_dt(lg), _p(lg), _p(out), _p(gt), _p(cm), ncm, 1 if align_corners else 0, F_, nc, h, w,
                                            H, W, _stream()), "upsample_argmax_cm")
    return out


def _same_memory(a: torch.Tensor, b: torch.Tensor) -> bool:
    """True when the bytes of two contiguous tensors overlap."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def labels_overlay(labels: torch.Tensor, table: torch.Tensor, frames: Optional[torch.Tensor] = None, edge_alpha: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 labels [n][H][W] -> uint8 RGB [n][H][W][3]: the colour table[label] = (r, g, b, a) (uint8 [256][4],
    utils.visualize.overlay_table) blended onto uint8 HWC `frames` [n][H][W][3] (None: onto black), out = (a c + (255 - a) s + 127) / 255
    per channel.  edge_alpha 0 .. 255 gives pixels whose label differs from a 4-neighbour's that alpha (outlines), None none.  `out`
    may be `frames` (in place), never memory of `labels`; returns out (include/stswin_hip.h, stswin_labels_overlay)."""
    if labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise StswinHipError(f"labels_overlay: labels must be contiguous uint8 [n][H][W], got {labels.dtype} {tuple(labels.shape)}")
    n, H, W = labels.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"labels_overlay: empty labels {tuple(labels.shape)}")
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 4) or not table.is_contiguous() or table.device != labels.device:
        raise StswinHipError(f"labels_overlay: table must be contiguous uint8 [256][4] on {labels.device}, got {table.dtype} "
                             f"{tuple(table.shape)} on {table.device}")
    for t, what in ((frames, "frames"), (out, "out")):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != (n, H, W, 3) or not t.is_contiguous() or t.device != labels.device):
            raise StswinHipError(f"labels_overlay: {what} must be contiguous uint8 [{n}][{H}][{W}][3] on {labels.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
    if edge_alpha is None:
        edge_alpha = -1
    elif not isinstance(edge_alpha, int) or not 0 <= edge_alpha <= 255:
        raise StswinHipError(f"labels_overlay: edge_alpha must be None or an int 0 .. 255, got {edge_alpha!r}")
    if out is None:
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=labels.device)
    elif _same_memory(out, labels):
        raise StswinHipError("labels_overlay: out shares memory with labels (only frames may be overwritten in place)")
    _check(load().stswin_labels_overlay(_p(labels), _p(frames), _p(table), _p(out), n, H, W, edge_alpha, _stream()), "labels_overlay")
    return out


def gt_decode(src: torch.Tensor, table: torch.Tensor, out_dtype: torch.dtype = torch.uint8, unmatched: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stored ground truth -> class indices [n][H][W] of out_dtype torch.uint8 (what labels_overlay reads) or torch.int64 (what
    upsample_argmax / upsample_argmax_cm read as gt).  src uint8 [n][H][W][3 | 4] with table uint8 [k][4] = (r, g, b, label), 1 <= k
    <= 256 (utils.groundtruth.colour_table): the label of the last row equal to the pixel's first three channels, 0 where none is,
    and such pixels counted per frame into `unmatched` (int32 [n], accumulated, None = not counted).  src uint8 [n][H][W] with table
    uint8 [256] (utils.groundtruth.remap_table): table[u].  `out` must not share memory with src; returns out
    (include/stswin_hip.h, stswin_gt_decode)."""
    if src.dtype != torch.uint8 or src.dim() not in (3, 4) or not src.is_contiguous() or (src.dim() == 4 and src.shape[3] not in (3, 4)):
        raise StswinHipError(f"gt_decode: src must be contiguous uint8 [n][H][W] or [n][H][W][3 | 4], got {src.dtype} {tuple(src.shape)}")
    n, H, W = src.shape[:3]
    ch = 1 if src.dim() == 3 else src.shape[3]
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"gt_decode: empty src {tuple(src.shape)}")
    if out_dtype not in (torch.uint8, torch.int64):
        raise StswinHipError(f"gt_decode: out_dtype must be torch.uint8 or torch.int64, got {out_dtype}")
    want = (256,) if ch == 1 else (table.shape[0] if table.dim() == 2 and 1 <= table.shape[0] <= 256 else -1, 4)
    if table.dtype != torch.uint8 or tuple(table.shape) != want or not table.is_contiguous() or table.device != src.device:
        form = "[256]" if ch == 1 else "[1 .. 256][4]"
        raise StswinHipError(f"gt_decode: the table of {ch}-channel ground truth must be contiguous uint8 {form} on {src.device}, got "
                             f"{table.dtype} {tuple(table.shape)} on {table.device}")
    if unmatched is not None and (unmatched.dtype != torch.int32 or tuple(unmatched.shape) != (n,) or not unmatched.is_contiguous()
                                  or unmatched.device != src.device):
        raise StswinHipError(f"gt_decode: unmatched must be contiguous int32 [{n}] on {src.device}, got {unmatched.dtype} "
                             f"{tuple(unmatched.shape)} on {unmatched.device}")
    if out is None:
        out = torch.empty(n, H, W, dtype=out_dtype, device=src.device)
    elif out.dtype != out_dtype or tuple(out.shape) != (n, H, W) or not out.is_contiguous() or out.device != src.device:
        raise StswinHipError(f"gt_decode: out must be contiguous {out_dtype} [{n}][{H}][{W}] on {src.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
    elif _same_memory(out, src):
        raise StswinHipError("gt_decode: out shares memory with src")
    _check(load().stswin_gt_decode(_p(src), _p(table), _p(out), _p(unmatched), n, H, W, ch, table.shape[0], out.element_size(),
                                   _stream()), "gt_decode")
    return out


def label_moments(labels: torch.Tensor, nc: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 labels [n][H][W] -> int64 [n][nc][10], per frame and class c < nc over the pixels (y, x) with that label: count, sum x,
    sum y, sum x^2, sum xy, sum y^2, max(W - x), max(H - y), max(x + 1), max(y + 1) (utils.instruments.label_moments is the numpy
    definition; an all-zero row is an absent class, labels >= nc are counted nowhere).  Without `out` the result starts from zeros; a
    given `out` is accumulated into (sums add, extents take the maximum) and must not share memory with labels; returns out
    (include/stswin_hip.h, stswin_label_moments)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise StswinHipError(f"label_moments: labels must be contiguous uint8 [n][H][W], got {got}")
    n, H, W = labels.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"label_moments: empty labels {tuple(labels.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"label_moments: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    if not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"label_moments: {nc!r} classes, the kernel takes 1 .. 64")
    if out is None:
        out = torch.zeros(n, nc, 10, dtype=torch.int64, device=labels.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (n, nc, 10) or not out.is_contiguous()
          or out.device != labels.device):
        got = f"{out.dtype} {tuple(out.shape)} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise StswinHipError(f"label_moments: out must be contiguous int64 [{n}][{nc}][10] on {labels.device}, got {got}")
    elif _same_memory(out, labels):
        raise StswinHipError("label_moments: out shares memory with labels")
    _check(load().stswin_label_moments(_p(labels), _p(out), n, H, W, nc, _stream()), "label_moments")
    return out


CC_TILE = (16, 64)          # stswin_label_components: (height, width) of the tile a workgroup labels in LDS ...
CC_CHUNK = 2048             # ... and the pixels of a raster chunk of its numbering pass (stswin_label_components_geometry gives the same)


def label_components_scratch(n: int, H: int, W: int) -> int:
    """Bytes of workspace hip.label_components needs for labels [n][H][W]."""
    b = int(load().stswin_label_components_scratch(n, H, W))
    if b < 0:
        raise StswinHipError(f"label_components: {n} maps of {H} x {W}, the kernel takes up to 16384 x 16384")
    return b


def label_components(labels: torch.Tensor, nc: int, connectivity: int = 8, skip=(), max_instances: int = 256, out=None,
                     workspace: Optional[torch.Tensor] = None):
    """uint8 labels [n][H][W] -> (components int32 [n][H][W], rows int64 [n][K][12], total int32 [n]), K = max_instances: the connected
    components (4- or 8-connectivity, within a frame) of the labels c < nc not in `skip`, numbered per frame by their first pixel in
    raster order; components holds each pixel's ordinal (-1: no component), total the frame's count, neither bounded by K; rows[f][i]
    for i < min(total[f], K) is [class, first pixel y W + x, then the ten integers of label_moments over the instance], zero from
    total[f] on (utils.instruments.label_components is the numpy definition, matched bit for bit, truncation included).  out: a triple
    of such buffers, written in full; workspace: uint8, >= label_components_scratch(n, H, W) bytes.  With both given the call
    allocates nothing and synchronises nothing (graph-capturable).  Returns the triple (include/stswin_hip.h,
    stswin_label_components)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise StswinHipError(f"label_components: labels must be contiguous uint8 [n][H][W], got {got}")
    if not labels.is_cuda:
        raise StswinHipError("label_components: labels must be on the GPU (no CPU path exists; utils.instruments.label_components is "
                             "the numpy definition)")
    n, H, W = labels.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"label_components: empty labels {tuple(labels.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"label_components: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"label_components: {nc!r} classes, the kernel takes 1 .. 64")
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (4, 8):
        raise StswinHipError(f"label_components: connectivity must be 4 or 8, got {connectivity!r}")
    try:
        skip = tuple(skip)
    except TypeError:
        skip = (skip,)
    if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 63 for c in skip):
        raise StswinHipError(f"label_components: skip holds classes 0 .. 63, got {skip!r}")
    K = max_instances
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 1024:
        raise StswinHipError(f"label_components: max_instances must be 1 .. 1024, got {K!r}")
    dev = labels.device
    want = (("components", torch.int32, (n, H, W)), ("rows", torch.int64, (n, K, 12)), ("total", torch.int32, (n,)))
    if out is None:
        out = tuple(torch.empty(shape, dtype=dt, device=dev) for _, dt, shape in want)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise StswinHipError("label_components: out must be the triple (components, rows, total)")
        for t, (what, dt, shape) in zip(out, want):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
                form = "".join(f"[{d}]" for d in shape)
                raise StswinHipError(f"label_components: {what} must be contiguous {dt} {form} on {dev}, got {got}")
    need = label_components_scratch(n, H, W)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != dev):
        got = f"{workspace.dtype} {tuple(workspace.shape)} on {workspace.device}" if isinstance(workspace, torch.Tensor) else type(workspace).__name__
        raise StswinHipError(f"label_components: workspace must be contiguous uint8 [bytes] on {dev}, got {got}")
    elif workspace.numel() < need:
        raise StswinHipError(f"label_components: a workspace of {workspace.numel()} bytes, {n} maps of {H} x {W} need {need}")
    elif workspace.data_ptr() % 4:
        raise StswinHipError("label_components: workspace must be 4-byte aligned")
    bufs = (("labels", labels), ("components", out[0]), ("rows", out[1]), ("total", out[2]), ("workspace", workspace))
    for i, (wa, a) in enumerate(bufs):
        for wb, b in bufs[i + 1:]:
            if _same_memory(a, b):
                raise StswinHipError(f"label_components: {wb} shares memory with {wa}")
    mask = 0
    for c in skip:
        mask |= 1 << c
    if mask >= 1 << 63:                      # (the mask travels in a C long: bit 63 is its sign bit)
        mask -= 1 << 64
    _check(load().stswin_label_components(_p(labels), _p(out[0]), _p(out[1]), _p(out[2]), n, H, W, nc, connectivity, mask, K,
                                          _p(workspace), workspace.numel(), _stream()), "label_components")
    return tuple(out)


TRACK_MAX_GAP = 1000000      # stswin_track_memory: the largest max_gap


def _track_shape(what: str, H, W, K) -> None:
    for name, v in (("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 16384:
            raise StswinHipError(f"{what}: {name} must be an int 1 .. 16384, got {v!r}")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 1024:
        raise StswinHipError(f"{what}: K must be an int 1 .. 1024, got {K!r}")


class TrackState:
    """What hip.track_instances keeps between the frames of a sequence, for maps [H][W] and K instances: one device buffer of
    stswin_track_state_bytes(H, W, K) bytes (the previous map, classes, areas and ids, the next id and the overlap counts; layout:
    include/stswin_hip.h).  Made reset: the first frame it sees is all births from id 0.  reset() starts the next sequence (a fill
    kernel on the current stream, graph-capturable).

    max_gap >= 1 (frames, up to 1000000): the state of the tracker with a memory (utils.instruments.MemoryTracker), which keeps a
    track alive for up to max_gap frames in which no instance was matched to it - stswin_track_memory_state_bytes(H, W, K) bytes (the
    tracks' slots, the table of the last frame's ordinals, the overlap counts and the memory map), sized and reset through the memory
    entry points.  memory=True takes that path with max_gap=0 too, where every unmatched track ends at once."""

    def __init__(self, H: int, W: int, K: int, device, max_gap: int = 0, memory: bool = False):
        _track_shape("TrackState", H, W, K)
        if isinstance(max_gap, bool) or not isinstance(max_gap, int) or not 0 <= max_gap <= TRACK_MAX_GAP:
            raise StswinHipError(f"TrackState: max_gap must be an int 0 .. {TRACK_MAX_GAP} (frames), got {max_gap!r}")
        if not isinstance(memory, bool):
            raise StswinHipError(f"TrackState: memory must be a bool, got {memory!r}")
        device = _device(device)
        if device.type != "cuda":
            raise StswinHipError("TrackState: the state lives on the GPU (utils.instruments.InstanceTracker is the numpy definition)")
        self.H, self.W, self.K, self.device = H, W, K, device
        self.max_gap, self.memory = max_gap, memory or max_gap > 0
        size = load().stswin_track_memory_state_bytes if self.memory else load().stswin_track_state_bytes
        self.bytes = int(size(H, W, K))
        if self.bytes < 0:
            raise StswinHipError(f"TrackState: {size.__name__}({H}, {W}, {K}) failed with code {self.bytes}")
        self.buffer = torch.empty(self.bytes, dtype=torch.uint8, device=device)      # (the caching allocator aligns to 512 bytes)
        self.reset()

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            if self.memory:
                _check(load().stswin_track_memory_reset(_p(self.buffer), self.bytes, self.H, self.W, self.K, _stream()), "track_memory_reset")
            else:
                _check(load().stswin_track_reset(_p(self.buffer), self.bytes, self.H, self.W, self.K, _stream()), "track_reset")


def track_instances(components: torch.Tensor, rows: torch.Tensor, total: torch.Tensor, state: TrackState, min_iou: int = 100,
                    same_class: bool = True, min_area: int = 1, out=None):
    """One frame of hip.label_components - components int32 [H][W], rows int64 [K][12], total int32 [1] (or a scalar tensor) - and the
    TrackState of its sequence -> (ids int32 [K], started int32 [1]): ids[j] is the track of instance j, carried over from the
    instance of the previous call that it overlaps best (intersection over union >= min_iou thousandths, the same class unless
    same_class=False, greedy in order of preference), a new id next, next + 1, ... for the participants left over, -1 for
    instances below min_area and rows past min(total, K); started = the ids handed out since the state's reset().  Frames go in
    frame order.  utils.instruments.InstanceTracker is the numpy definition, matched bit for bit.  out: the pair (ids, started),
    written in full; with it the call allocates nothing, and it never synchronises (graph-capturable).  Two launches
    (include/stswin_hip.h, stswin_track_instances).

    A state made with max_gap >= 1 (or memory=True) goes through the tracker with a memory instead: a track that no instance was
    matched to stays alive for up to state.max_gap frames, and instances are matched against the mask each track had when it was last
    seen.  utils.instruments.MemoryTracker is the numpy definition, matched bit for bit.  Three launches (stswin_track_memory)."""
    if not isinstance(state, TrackState):
        raise StswinHipError(f"track_instances: state must be a hip.TrackState, got {type(state).__name__}")
    H, W, K, dev = state.H, state.W, state.K, state.device
    want = [("components", components, torch.int32, (H, W)), ("rows", rows, torch.int64, (K, 12)), ("total", total, torch.int32, None)]
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise StswinHipError("track_instances: out must be the pair (ids, started)")
        want += [("ids", out[0], torch.int32, (K,)), ("started", out[1], torch.int32, (1,))]
    for what, t, dt, shape in want:
        ok = isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.device == dev
        if ok:
            ok = tuple(t.shape) == shape if shape is not None else t.numel() == 1 and t.dim() <= 1
        if not ok:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            form = "".join(f"[{d}]" for d in shape) if shape is not None else "[1]"
            raise StswinHipError(f"track_instances: {what} must be contiguous {dt} {form} on {dev} (a state of {H} x {W} maps and "
                                 f"{K} instances), got {got}")
    if isinstance(min_iou, bool) or not isinstance(min_iou, int) or not 0 <= min_iou <= 1000:
        raise StswinHipError(f"track_instances: min_iou must be an int 0 .. 1000 (thousandths), got {min_iou!r}")
    if not isinstance(same_class, bool):
        raise StswinHipError(f"track_instances: same_class must be a bool, got {same_class!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 1:
        raise StswinHipError(f"track_instances: min_area must be an int >= 1, got {min_area!r}")
    if out is None:
        out = (torch.empty(K, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    bufs = (("components", components), ("rows", rows), ("total", total), ("state", state.buffer), ("ids", out[0]), ("started", out[1]))
    for i, (wa, a) in enumerate(bufs):
        for wb, b in bufs[i + 1:]:
            if _same_memory(a, b):
                raise StswinHipError(f"track_instances: {wb} shares memory with {wa}")
    if state.memory:
        _check(load().stswin_track_memory(_p(components), _p(rows), _p(total), _p(state.buffer), state.bytes, H, W, K, state.max_gap, min_iou,
                                          int(same_class), min_area, _p(out[0]), _p(out[1]), _stream()), "track_memory")
    else:
        _check(load().stswin_track_instances(_p(components), _p(rows), _p(total), _p(state.buffer), state.bytes, H, W, K, min_iou,
                                             int(same_class), min_area, _p(out[0]), _p(out[1]), _stream()), "track_instances")
    return tuple(out)


RLE_MAX_RUNS = 1 << 20       # stswin_rle_encode: the largest cap


def rle_geometry():
    """(rows of a segment, columns of a workgroup's band, pixels per thread and row) of stswin_rle_encode."""
    return tuple(int(load().stswin_rle_geometry(i)) for i in range(3))


def rle_encode_scratch(n: int, H: int, W: int) -> int:
    """Bytes of workspace hip.rle_encode needs for maps [n][H][W]."""
    b = int(load().stswin_rle_encode_scratch(n, H, W))
    if b < 0:
        raise StswinHipError(f"rle_encode: {n} maps of {H} x {W}, the kernel takes up to 16384 x 16384")
    return b


def rle_encode(maps: torch.Tensor, cap: int, out=None, workspace: Optional[torch.Tensor] = None):
    """uint8 (a label map) or int32 (hip.label_components' map) maps [n][H][W] -> (runs int32 [n][cap][2], count int32 [n]): per frame
    the runs of its column-major reading v[p] = maps[f][y][x], p = x H + y (COCO's order).  count[f] is the number of runs, not bounded
    by cap; runs[f][i] = (p_i, v[p_i]) for i < min(count[f], cap) in ascending p, zero from there on - the first cap runs are kept
    (utils.rle.encode is the numpy definition, matched bit for bit).  out: the pair (runs, count), written in full; workspace: uint8, >=
    rle_encode_scratch(n, H, W) bytes.  With both given the call allocates nothing, and it never synchronises (graph-capturable).
    Three launches.  Returns the pair (include/stswin_hip.h, stswin_rle_encode)."""
    if not isinstance(maps, torch.Tensor) or maps.dtype not in (torch.uint8, torch.int32) or maps.dim() != 3 or not maps.is_contiguous():
        got = f"{maps.dtype} {tuple(maps.shape)}" if isinstance(maps, torch.Tensor) else type(maps).__name__
        raise StswinHipError(f"rle_encode: maps must be contiguous uint8 or int32 [n][H][W], got {got}")
    if not maps.is_cuda:
        raise StswinHipError("rle_encode: maps must be on the GPU (no CPU path exists; utils.rle.encode is the numpy definition)")
    n, H, W = maps.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"rle_encode: empty maps {tuple(maps.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"rle_encode: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap <= RLE_MAX_RUNS:
        raise StswinHipError(f"rle_encode: cap must be an int 1 .. {RLE_MAX_RUNS}, got {cap!r}")
    dev = maps.device
    want = (("runs", torch.int32, (n, cap, 2)), ("count", torch.int32, (n,)))
    if out is None:
        out = tuple(torch.empty(shape, dtype=dt, device=dev) for _, dt, shape in want)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise StswinHipError("rle_encode: out must be the pair (runs, count)")
        for t, (what, dt, shape) in zip(out, want):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
                form = "".join(f"[{d}]" for d in shape)
                raise StswinHipError(f"rle_encode: {what} must be contiguous {dt} {form} on {dev}, got {got}")
    need = rle_encode_scratch(n, H, W)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != dev):
        got = f"{workspace.dtype} {tuple(workspace.shape)} on {workspace.device}" if isinstance(workspace, torch.Tensor) else type(workspace).__name__
        raise StswinHipError(f"rle_encode: workspace must be contiguous uint8 [bytes] on {dev}, got {got}")
    elif workspace.numel() < need:
        raise StswinHipError(f"rle_encode: a workspace of {workspace.numel()} bytes, {n} maps of {H} x {W} need {need}")
    elif workspace.data_ptr() % 4:
        raise StswinHipError("rle_encode: workspace must be 4-byte aligned")
    bufs = (("maps", maps), ("runs", out[0]), ("count", out[1]), ("workspace", workspace))
    for i, (wa, a) in enumerate(bufs):
        for wb, b in bufs[i + 1:]:
            if _same_memory(a, b):
                raise StswinHipError(f"rle_encode: {wb} shares memory with {wa}")
    _check(load().stswin_rle_encode(_p(maps), maps.element_size(), _p(out[0]), _p(out[1]), n, H, W, cap, _p(workspace), workspace.numel(),
                                    _stream()), "rle_encode")
    return tuple(out)


def boundary_geometry():
    """(rows, columns of the tile a workgroup of the query pass owns, columns of a workgroup and rows of a segment of the column pass)
    of stswin_boundary_counts."""
    return tuple(int(load().stswin_boundary_geometry(i)) for i in range(4))


def boundary_scratch(n: int, H: int, W: int, nc: int) -> int:
    """Bytes of workspace hip.boundary_counts needs for maps [n][H][W] of nc classes: 16 n (ceil(H / 64) W + 1) + 2 n H W (2 nc + 1)."""
    b = int(load().stswin_boundary_scratch(n, H, W, nc))
    if b == -1872:
        raise StswinHipError(f"boundary_counts: nc = {nc!r} classes, the kernel takes 1 .. 64")
    if b < 0:
        raise StswinHipError(f"boundary_counts: {n} maps of {H} x {W}, the kernel takes up to 16384 x 16384")
    return b


def boundary_counts(gt: torch.Tensor, pred: torch.Tensor, nc: int, bins: int = 32, skip=(), out: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 gt [n][H][W] and uint8 pred [n][H][W] -> int32 [n][nc][2][2 + bins]: per frame, class and direction (0: gt's contour
    measured against pred's, 1: pred's against gt's) the size of the contour, the largest squared distance to the other contour (-1:
    either one is empty) and the contour pixels per ceil(distance), the last bin open-ended; the rows of the classes in `skip` are zero
    (utils.boundary.boundary_counts is the numpy definition, matched bit for bit; utils.boundary.BoundaryScores reads NSD and
    Hausdorff distances from the rows).  out: written in full; workspace: uint8, >= boundary_scratch(n, H, W, nc) bytes.  With both
    given the call allocates nothing, and it never synchronises (graph-capturable).  Five launches.  Returns out
    (include/stswin_hip.h, stswin_boundary_counts)."""
    for what, t, dt in (("gt", gt, torch.int64), ("pred", pred, torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 3 or not t.is_contiguous():
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise StswinHipError(f"boundary_counts: {what} must be contiguous {dt} [n][H][W], got {got}")
        if not t.is_cuda:
            raise StswinHipError(f"boundary_counts: {what} must be on the GPU (no CPU path exists; utils.boundary.boundary_counts is the "
                                 "numpy definition)")
    n, H, W = gt.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"boundary_counts: empty gt {tuple(gt.shape)}")
    if tuple(pred.shape) != (n, H, W) or pred.device != gt.device:
        raise StswinHipError(f"boundary_counts: pred must be [{n}][{H}][{W}] on {gt.device} as gt is, got {tuple(pred.shape)} on {pred.device}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"boundary_counts: a {H} x {W} gt, the kernel takes up to 16384 x 16384")
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"boundary_counts: nc = {nc!r} classes, the kernel takes 1 .. 64")
    if isinstance(bins, bool) or not isinstance(bins, int) or not 2 <= bins <= 256:
        raise StswinHipError(f"boundary_counts: bins must be an int 2 .. 256, got {bins!r}")
    try:
        skip = tuple(skip)
    except TypeError:
        skip = (skip,)
    if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 63 for c in skip):
        raise StswinHipError(f"boundary_counts: skip holds classes 0 .. 63, got {skip!r}")
    dev = gt.device
    shape = (n, nc, 2, 2 + bins)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        got = f"{out.dtype} {tuple(out.shape)} on {out.device}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise StswinHipError(f"boundary_counts: out must be contiguous torch.int32 [{n}][{nc}][2][{2 + bins}] on {dev}, got {got}")
    need = boundary_scratch(n, H, W, nc)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != dev):
        got = f"{workspace.dtype} {tuple(workspace.shape)} on {workspace.device}" if isinstance(workspace, torch.Tensor) else type(workspace).__name__
        raise StswinHipError(f"boundary_counts: workspace must be contiguous uint8 [bytes] on {dev}, got {got}")
    elif workspace.numel() < need:
        raise StswinHipError(f"boundary_counts: a workspace of {workspace.numel()} bytes, {n} maps of {H} x {W} and {nc} classes need {need}")
    elif workspace.data_ptr() % 8:
        raise StswinHipError("boundary_counts: workspace must be 8-byte aligned")
    bufs = (("gt", gt), ("pred", pred), ("out", out), ("workspace", workspace))
    for i, (wa, a) in enumerate(bufs):
        for wb, b in bufs[i + 1:]:
            if _same_memory(a, b):
                raise StswinHipError(f"boundary_counts: {wb} shares memory with {wa}")
    mask = 0
    for c in skip:
        mask |= 1 << c
    if mask >= 1 << 63:                      # (the mask travels in a C long: bit 63 is its sign bit)
        mask -= 1 << 64
    _check(load().stswin_boundary_counts(_p(gt), _p(pred), _p(out), n, H, W, nc, bins, mask, _p(workspace), workspace.numel(), _stream()),
           "boundary_counts")
    return out


def _got(t) -> str:
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__


def upsample_confidence(logits: torch.Tensor, labels: torch.Tensor, align_corners: bool = True,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NCHW logits [F][nc][h][w] (bf16 / fp32, nc <= 64) and uint8 labels [F][H][W] -> uint8 [F][H][W]: the softmax probability, over
    the classes of the bilinear resize of the logits to (H, W) (align_corners as F.interpolate), of each pixel's label, as min(255,
    floor(255 p + 0.5)); 0 where the label is >= nc.  The resize is the one of upsample_argmax (align_corners=True) and
    upsample_argmax_cm, so for their labels it is the largest probability (utils.confidence.upsample_confidence is the numpy
    definition).  out: written in full; with it the call allocates nothing, and it never synchronises (graph-capturable).  One launch.
    Returns out (include/stswin_hip.h, stswin_upsample_confidence)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.dtype not in (torch.bfloat16, torch.float32) or not logits.is_contiguous():
        raise StswinHipError(f"upsample_confidence: logits must be contiguous bf16 or fp32 [F][nc][h][w], got {_got(logits)}")
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.dtype != torch.uint8 or not labels.is_contiguous():
        raise StswinHipError(f"upsample_confidence: labels must be contiguous uint8 [F][H][W], got {_got(labels)}")
    if not logits.is_cuda or not labels.is_cuda:
        raise StswinHipError("upsample_confidence: logits and labels must be on the GPU (no CPU path exists; "
                             "utils.confidence.upsample_confidence is the numpy definition)")
    F_, nc, h, w = logits.shape
    if labels.shape[0] != F_ or labels.device != logits.device:
        raise StswinHipError(f"upsample_confidence: labels must be [{F_}][H][W] on {logits.device} as the logits are, got {_got(labels)}")
    if logits.numel() == 0 or labels.numel() == 0:
        raise StswinHipError(f"upsample_confidence: empty logits {tuple(logits.shape)} or labels {tuple(labels.shape)}")
    if not 1 <= nc <= 64:
        raise StswinHipError(f"upsample_confidence: {nc} classes, the kernel takes 1 .. 64")
    if h * w >= 1 << 31:
        raise StswinHipError(f"upsample_confidence: logits of {h} x {w}, the kernel takes h w < 2^31")
    H, W = labels.shape[1:]
    if out is None:
        out = torch.empty(F_, H, W, dtype=torch.uint8, device=labels.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (F_, H, W) or not out.is_contiguous()
          or out.device != labels.device):
        raise StswinHipError(f"upsample_confidence: out must be contiguous uint8 [{F_}][{H}][{W}] on {labels.device}, got {_got(out)}")
    elif _same_memory(out, labels) or _same_memory(out, logits):
        raise StswinHipError("upsample_confidence: out shares memory with labels or logits")
    _check(load().stswin_upsample_confidence(_dt(logits), _p(logits), _p(labels), _p(out), 1 if align_corners else 0, F_, nc, h, w, H, W,
                                             _stream()), "upsample_confidence")
    return out


def confidence_sums(maps: torch.Tensor, conf: torch.Tensor, K: int, low: int = 128, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 (a label map) or int32 (hip.label_components' map, -1 = none) maps [n][H][W] and uint8 conf [n][H][W] -> int64 [n][K][3]:
    per frame and map value i in [0, K) the number of its pixels, the sum of their conf and the number of them with conf < low (0 ..
    256); other values are counted nowhere (utils.confidence.confidence_sums is the numpy definition, matched bit for bit).  out:
    written in full - cleared by a fill kernel, so a second call overwrites; with it the call allocates nothing, and it never
    synchronises (graph-capturable).  Two launches.  Returns out (include/stswin_hip.h, stswin_confidence_sums)."""
    if not isinstance(maps, torch.Tensor) or maps.dtype not in (torch.uint8, torch.int32) or maps.dim() != 3 or not maps.is_contiguous():
        raise StswinHipError(f"confidence_sums: maps must be contiguous uint8 or int32 [n][H][W], got {_got(maps)}")
    if not isinstance(conf, torch.Tensor) or conf.dtype != torch.uint8 or conf.shape != maps.shape or not conf.is_contiguous():
        raise StswinHipError(f"confidence_sums: conf must be contiguous uint8 {tuple(maps.shape)} as the maps are, got {_got(conf)}")
    if not maps.is_cuda or not conf.is_cuda:
        raise StswinHipError("confidence_sums: maps and conf must be on the GPU (no CPU path exists; utils.confidence.confidence_sums "
                             "is the numpy definition)")
    if conf.device != maps.device:
        raise StswinHipError(f"confidence_sums: conf must be on {maps.device} as the maps are, got {conf.device}")
    n, H, W = maps.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"confidence_sums: empty maps {tuple(maps.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"confidence_sums: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 1024:
        raise StswinHipError(f"confidence_sums: K must be an int 1 .. 1024, got {K!r}")
    if isinstance(low, bool) or not isinstance(low, int) or not 0 <= low <= 256:
        raise StswinHipError(f"confidence_sums: low must be an int 0 .. 256, got {low!r}")
    if out is None:
        out = torch.empty(n, K, 3, dtype=torch.int64, device=maps.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (n, K, 3) or not out.is_contiguous()
          or out.device != maps.device):
        raise StswinHipError(f"confidence_sums: out must be contiguous int64 [{n}][{K}][3] on {maps.device}, got {_got(out)}")
    elif _same_memory(out, maps) or _same_memory(out, conf):
        raise StswinHipError("confidence_sums: out shares memory with maps or conf")
    _check(load().stswin_confidence_sums(_p(maps), maps.element_size(), _p(conf), _p(out), K, low, n, H, W, _stream()), "confidence_sums")
    return out


def instance_parts_geometry():
    """(tile height, tile width, on-chip key slots) of hip.instance_parts (stswin_instance_parts_geometry)."""
    geo = load().stswin_instance_parts_geometry
    return geo(0), geo(1), geo(2)


def instance_parts(labels: torch.Tensor, components: torch.Tensor, K: int, nc: int, out=None):
    """uint8 labels [n][H][W] and int32 components [n][H][W] (hip.label_components' map, -1 = none) -> (parts int64 [n][K][nc][10],
    contacts int64 [n][K][nc]): per frame, instance ordinal i < K and class c < nc the ten integers of label_moments over the pixels
    with components == i and labels == c, and the number of pixel edges between instance i and pixels of class c outside it (p in i, q
    one of p's four neighbours with components[q] != i and labels[q] == c).  Ordinals -1 and >= K are nobody's, labels >= nc count
    nowhere (utils.instruments.instance_parts is the numpy definition, matched bit for bit).  out: the pair of such buffers, written
    in full - cleared by a fill kernel, so a second call overwrites; with it the call allocates nothing, and it never synchronises
    (graph-capturable).  Three launches.  Returns the pair (include/stswin_hip.h, stswin_instance_parts)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise StswinHipError(f"instance_parts: labels must be contiguous uint8 [n][H][W], got {_got(labels)}")
    if (not isinstance(components, torch.Tensor) or components.dtype != torch.int32 or components.shape != labels.shape
            or not components.is_contiguous()):
        raise StswinHipError(f"instance_parts: components must be contiguous int32 {tuple(labels.shape)} as the labels are, got "
                             f"{_got(components)}")
    if not labels.is_cuda or not components.is_cuda:
        raise StswinHipError("instance_parts: labels and components must be on the GPU (no CPU path exists; "
                             "utils.instruments.instance_parts is the numpy definition)")
    if components.device != labels.device:
        raise StswinHipError(f"instance_parts: components must be on {labels.device} as the labels are, got {components.device}")
    n, H, W = labels.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"instance_parts: empty labels {tuple(labels.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"instance_parts: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 1024:
        raise StswinHipError(f"instance_parts: K must be an int 1 .. 1024, got {K!r}")
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"instance_parts: {nc!r} classes, the kernel takes 1 .. 64")
    dev = labels.device
    want = (("parts", (n, K, nc, 10)), ("contacts", (n, K, nc)))
    if out is None:
        out = tuple(torch.empty(shape, dtype=torch.int64, device=dev) for _, shape in want)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise StswinHipError("instance_parts: out must be the pair (parts, contacts)")
        for t, (what, shape) in zip(out, want):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                form = "".join(f"[{d}]" for d in shape)
                raise StswinHipError(f"instance_parts: {what} must be contiguous int64 {form} on {dev}, got {_got(t)}")
        bufs = (("labels", labels), ("components", components), ("parts", out[0]), ("contacts", out[1]))
        for i, (wa, a) in enumerate(bufs[:3]):
            for wb, b in bufs[max(i + 1, 2):]:
                if _same_memory(a, b):
                    raise StswinHipError(f"instance_parts: {wb} shares memory with {wa}")
    _check(load().stswin_instance_parts(_p(labels), _p(components), _p(out[0]), _p(out[1]), n, H, W, nc, K, _stream()), "instance_parts")
    return tuple(out)


def instance_clearance_geometry():
    """(rows, columns of the tile a workgroup of the query pass owns, columns of a workgroup and rows of a segment of the column pass,
    columns a lane searches to each side before the wave searches together, 64 a step, pixels of a row the wave still takes one by
    one) of hip.instance_clearance (stswin_instance_clearance_geometry)."""
    geo = load().stswin_instance_clearance_geometry
    return tuple(int(geo(i)) for i in range(6))


def instance_clearance_scratch(n: int, H: int, W: int, nc: int, K: int) -> int:
    """Bytes of workspace hip.instance_clearance needs for maps [n][H][W] of nc classes and K instances:
    8 n (ceil(H / 64) W + 1 + K nc + K) + n H W (2 nc + 1)."""
    for what, v in (("n", n), ("H", H), ("W", W), ("nc", nc), ("K", K)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise StswinHipError(f"instance_clearance: {what} must be an int, got {v!r}")
    b = int(load().stswin_instance_clearance_scratch(n, H, W, nc, K))
    if b == -1922:
        raise StswinHipError(f"instance_clearance: nc = {nc!r} classes, the kernel takes 1 .. 64")
    if b == -1923:
        raise StswinHipError(f"instance_clearance: K must be an int 1 .. 1024, got {K!r}")
    if b < 0:
        raise StswinHipError(f"instance_clearance: {n} maps of {H} x {W}, the kernel takes up to 16384 x 16384")
    return b


def instance_clearance(labels: torch.Tensor, components: torch.Tensor, K: int, nc: int, targets=None, max_distance: Optional[int] = None,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 labels [n][H][W] and int32 components [n][H][W] (hip.label_components' map, -1 = none) -> int64 [n][K][nc][3]: per frame,
    instance ordinal i < K and class c < nc the triple (d2, p, q) - d2 the smallest squared Euclidean pixel distance between a pixel
    with components == i and a pixel with labels == c, p = y W + x the first pixel of the instance in raster order that reaches it, q
    the first pixel of the class at that distance from p - or (-1, -1, -1) where the instance or the class is empty, c is not in
    `targets` (default: every class), the instance itself holds a pixel of class c (own classes are not measured) or d2 >
    max_distance^2.  Ordinals -1 and >= K are nobody's, labels >= nc are nowhere (utils.instruments.instance_clearance is the numpy
    definition, matched bit for bit).  out: written in full, a second call overwrites; workspace: uint8, 8-byte aligned, >=
    instance_clearance_scratch(n, H, W, nc, K) bytes.  With both given the call allocates nothing, and it never synchronises
    (graph-capturable).  Six launches.  Returns out (include/stswin_hip.h, stswin_instance_clearance)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise StswinHipError(f"instance_clearance: labels must be contiguous uint8 [n][H][W], got {_got(labels)}")
    if (not isinstance(components, torch.Tensor) or components.dtype != torch.int32 or components.shape != labels.shape
            or not components.is_contiguous()):
        raise StswinHipError(f"instance_clearance: components must be contiguous int32 {tuple(labels.shape)} as the labels are, got "
                             f"{_got(components)}")
    if not labels.is_cuda or not components.is_cuda:
        raise StswinHipError("instance_clearance: labels and components must be on the GPU (no CPU path exists; "
                             "utils.instruments.instance_clearance is the numpy definition)")
    if components.device != labels.device:
        raise StswinHipError(f"instance_clearance: components must be on {labels.device} as the labels are, got {components.device}")
    n, H, W = labels.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"instance_clearance: empty labels {tuple(labels.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"instance_clearance: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 1024:
        raise StswinHipError(f"instance_clearance: K must be an int 1 .. 1024, got {K!r}")
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"instance_clearance: nc = {nc!r} classes, the kernel takes 1 .. 64")
    if targets is None:
        targets = range(nc)
    try:
        targets = tuple(targets)
    except TypeError:
        targets = (targets,)
    if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < nc for c in targets):
        raise StswinHipError(f"instance_clearance: targets holds classes 0 .. {nc - 1}, got {targets!r}")
    if max_distance is not None and (isinstance(max_distance, bool) or not isinstance(max_distance, int) or max_distance < 0):
        raise StswinHipError(f"instance_clearance: max_distance must be None or an int >= 0 (pixels), got {max_distance!r}")
    dev = labels.device
    shape = (n, K, nc, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise StswinHipError(f"instance_clearance: out must be contiguous int64 [{n}][{K}][{nc}][3] on {dev}, got {_got(out)}")
    need = instance_clearance_scratch(n, H, W, nc, K)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != dev):
        raise StswinHipError(f"instance_clearance: workspace must be contiguous uint8 [bytes] on {dev}, got {_got(workspace)}")
    elif workspace.numel() < need:
        raise StswinHipError(f"instance_clearance: a workspace of {workspace.numel()} bytes, {n} maps of {H} x {W}, {nc} classes and {K} "
                             f"instances need {need}")
    elif workspace.data_ptr() % 8:
        raise StswinHipError("instance_clearance: workspace must be 8-byte aligned")
    bufs = (("labels", labels), ("components", components), ("out", out), ("workspace", workspace))
    for i, (wa, a) in enumerate(bufs[:3]):
        for wb, b in bufs[max(i + 1, 2):]:
            if _same_memory(a, b):
                raise StswinHipError(f"instance_clearance: {wb} shares memory with {wa}")
    mask = 0
    for c in targets:
        mask |= 1 << c
    if mask >= 1 << 63:                      # (the mask travels in a C long: bit 63 is its sign bit)
        mask -= 1 << 64
    max_d2 = -1 if max_distance is None else min(max_distance * max_distance, 1 << 30)       # (every d2 is < 2^30)
    _check(load().stswin_instance_clearance(_p(labels), _p(components), _p(out), n, H, W, nc, K, mask, max_d2, _p(workspace),
                                            workspace.numel(), _stream()), "instance_clearance")
    return out


def labels_clean_geometry():
    """(vote tile height, vote tile width, raster chunk of the numbering pass, slots of the on-chip vote table) of hip.labels_clean
    (stswin_labels_clean_geometry)."""
    geo = load().stswin_labels_clean_geometry
    return int(geo(0)), int(geo(1)), int(geo(2)), int(geo(3))


def _clean_ints(fn: str, nc, max_small) -> None:
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"{fn}: {nc!r} classes, the kernel takes 1 .. 64")
    if isinstance(max_small, bool) or not isinstance(max_small, int) or not 1 <= max_small <= 65536:
        raise StswinHipError(f"{fn}: max_small must be an int 1 .. 65536, got {max_small!r}")


def labels_clean_scratch(n: int, H: int, W: int, nc: int, max_small: int = 4096) -> int:
    """Bytes of workspace hip.labels_clean needs for labels [n][H][W] of nc classes."""
    _clean_ints("labels_clean", nc, max_small)
    b = int(load().stswin_labels_clean_scratch(n, H, W, nc, max_small))
    if b < 0:
        raise StswinHipError(f"labels_clean: {n} maps of {H} x {W}, the kernel takes up to 16384 x 16384")
    return b


def labels_clean(labels: torch.Tensor, nc: int, min_area: int, connectivity: int = 8, keep=(), max_small: int = 4096,
                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """uint8 labels [n][H][W] -> (out uint8 [n][H][W], stats int32 [n][2]): the label map with its specks removed and its small holes
    filled.  A component (4- or 8-connectivity, every class c < nc) of fewer than min_area pixels whose class is not in `keep` is small
    and takes the class that most of its pixel edges towards stable pixels - those of components that are not small - lead to, the
    smallest class on a tie, its own without such an edge; of a frame's small components, numbered by their first pixel in raster
    order, the first max_small can change.  stats[f] = (small components of frame f, not bounded by max_small; pixels whose label
    changed).  utils.instruments.clean_labels is the numpy definition, matched bit for bit, truncation included.  out: such a buffer,
    written in full; workspace: uint8, >= labels_clean_scratch(n, H, W, nc, max_small) bytes.  With both given the call allocates only
    stats and synchronises nothing (graph-capturable).  Returns (out, stats) (include/stswin_hip.h, stswin_labels_clean)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise StswinHipError(f"labels_clean: labels must be contiguous uint8 [n][H][W], got {_got(labels)}")
    if not labels.is_cuda:
        raise StswinHipError("labels_clean: labels must be on the GPU (no CPU path exists; utils.instruments.clean_labels is the numpy "
                             "definition)")
    n, H, W = labels.shape
    if n <= 0 or H <= 0 or W <= 0:
        raise StswinHipError(f"labels_clean: empty labels {tuple(labels.shape)}")
    if H > 16384 or W > 16384:
        raise StswinHipError(f"labels_clean: a {H} x {W} map, the kernel takes up to 16384 x 16384")
    _clean_ints("labels_clean", nc, max_small)
    if isinstance(min_area, bool) or not isinstance(min_area, int) or not 2 <= min_area <= 1 << 30:
        raise StswinHipError(f"labels_clean: min_area must be an int 2 .. 2^30, got {min_area!r}")
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (4, 8):
        raise StswinHipError(f"labels_clean: connectivity must be 4 or 8, got {connectivity!r}")
    try:
        keep = tuple(keep)
    except TypeError:
        keep = (keep,)
    if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 63 for c in keep):
        raise StswinHipError(f"labels_clean: keep holds classes 0 .. 63, got {keep!r}")
    dev = labels.device
    if out is None:
        out = torch.empty_like(labels)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or not out.is_contiguous()
          or out.device != dev):
        raise StswinHipError(f"labels_clean: out must be contiguous uint8 [{n}][{H}][{W}] on {dev}, got {_got(out)}")
    need = labels_clean_scratch(n, H, W, nc, max_small)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != dev):
        raise StswinHipError(f"labels_clean: workspace must be contiguous uint8 [bytes] on {dev}, got {_got(workspace)}")
    elif workspace.numel() < need:
        raise StswinHipError(f"labels_clean: a workspace of {workspace.numel()} bytes, {n} maps of {H} x {W} need {need}")
    elif workspace.data_ptr() % 4:
        raise StswinHipError("labels_clean: workspace must be 4-byte aligned")
    bufs = (("labels", labels), ("out", out), ("workspace", workspace))
    for i, (wa, a) in enumerate(bufs):
        for wb, b in bufs[i + 1:]:
            if _same_memory(a, b):
                raise StswinHipError(f"labels_clean: {wb} shares memory with {wa}")
    stats = torch.empty(n, 2, dtype=torch.int32, device=dev)
    mask = 0
    for c in keep:
        mask |= 1 << c
    if mask >= 1 << 63:                      # (the mask travels in a C long: bit 63 is its sign bit)
        mask -= 1 << 64
    _check(load().stswin_labels_clean(_p(labels), _p(out), _p(stats), n, H, W, nc, connectivity, mask, min_area, max_small,
                                      _p(workspace), workspace.numel(), _stream()), "labels_clean")
    return out, stats


def labels_score(labels: torch.Tensor, gt: torch.Tensor, nc: int, counts: Optional[torch.Tensor] = None,
                 cm: Optional[torch.Tensor] = None):
    """uint8 labels [n][H][W] and int64 gt [n][H][W] -> (counts, cm): what the fused label launches count, from a label map that
    already exists.  counts int32 [n][3][nc] (made of zeros when neither is given; a given one is added to): per frame and class
    |gt == c|, |labels == c|, |gt == c and labels == c|, the integers of hip.upsample_argmax.  cm int64 [ncm][ncm]: every pixel with
    gt and label in [0, ncm) adds 1 to cm[gt][label]; accumulated, not cleared, as hip.upsample_argmax_cm does.  One launch, no
    synchronisation (include/stswin_hip.h, stswin_labels_score)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise StswinHipError(f"labels_score: labels must be contiguous uint8 [n][H][W], got {_got(labels)}")
    if not labels.is_cuda:
        raise StswinHipError("labels_score: labels must be on the GPU (no CPU path exists)")
    n, H, W = labels.shape
    dev = labels.device
    if n <= 0 or H <= 0 or W <= 0 or H > 16384 or W > 16384:
        raise StswinHipError(f"labels_score: labels {tuple(labels.shape)}, the kernel takes 1 .. 16384 x 1 .. 16384")
    if (not isinstance(gt, torch.Tensor) or gt.dtype != torch.int64 or tuple(gt.shape) != (n, H, W) or not gt.is_contiguous()
            or gt.device != dev):
        raise StswinHipError(f"labels_score: gt must be contiguous int64 [{n}][{H}][{W}] on {dev}, got {_got(gt)}")
    if isinstance(nc, bool) or not isinstance(nc, int) or not 1 <= nc <= 64:
        raise StswinHipError(f"labels_score: {nc!r} classes, the kernel takes 1 .. 64")
    if counts is None and cm is None:
        counts = torch.zeros(n, 3, nc, dtype=torch.int32, device=dev)
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or tuple(counts.shape) != (n, 3, nc)
                               or not counts.is_contiguous() or counts.device != dev):
        raise StswinHipError(f"labels_score: counts must be contiguous int32 [{n}][3][{nc}] on {dev}, got {_got(counts)}")
    ncm = 0
    if cm is not None:
        if (not isinstance(cm, torch.Tensor) or cm.dtype != torch.int64 or cm.dim() != 2 or cm.shape[0] != cm.shape[1]
                or not cm.is_contiguous() or cm.device != dev):
            raise StswinHipError(f"labels_score: cm must be contiguous int64 [ncm][ncm] on {dev}, got {_got(cm)}")
        ncm = cm.shape[0]
        if not 1 <= ncm <= 64:
            raise StswinHipError(f"labels_score: a {ncm} x {ncm} matrix, the kernel takes 1 .. 64 classes")
    for what, t in (("counts", counts), ("cm", cm)):
        if t is not None and (_same_memory(t, labels) or _same_memory(t, gt)):
            raise StswinHipError(f"labels_score: {what} shares memory with labels or gt")
    _check(load().stswin_labels_score(_p(labels), _p(gt), _p(counts), _p(cm), ncm, n, H, W, nc, _stream()), "labels_score")
    return counts, cm


YUV_NV12, YUV_UYVY = 0, 1                    # stswin_yuv_to_rgb's `format` (plain integers in the header's comment, not #defines)
YUV_REPLICATE, YUV_LINEAR = 0, 1               # ... and its `chroma`
_YUV_FORMATS = {"nv12": YUV_NV12, "uyvy": YUV_UYVY}
_YUV_CHROMA = {"replicate": YUV_REPLICATE, "linear": YUV_LINEAR}


def _yuv_matrix(matrix: torch.Tensor, device, what: str) -> None:
    if (not isinstance(matrix, torch.Tensor) or matrix.dtype != torch.int32 or tuple(matrix.shape) != (3, 4) or not matrix.is_contiguous()
            or matrix.device != device):
        got = f"{matrix.dtype} {tuple(matrix.shape)} on {matrix.device}" if isinstance(matrix, torch.Tensor) else type(matrix).__name__
        raise StswinHipError(f"{what}: matrix must be contiguous int32 [3][4] on {device} (utils.yuv), got {got}")


def yuv_to_rgb(src: torch.Tensor, matrix: torch.Tensor, fmt: str = "nv12", chroma: str = "replicate",
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raw video frames -> uint8 RGB [n][Hs][Ws][3]: fmt="nv12" src uint8 [n][3 Hs / 2][Ws] (luma rows, then rows of (U, V) pairs),
    fmt="uyvy" src uint8 [n][Hs][Ws][2] (U, Y0, V, Y1 per pixel pair), Hs (nv12) and Ws even.  matrix int32 [3][4] on the device
    (utils.yuv.to_rgb_matrix); chroma="replicate" | "linear" as utils.yuv.yuv_to_rgb defines them, which this equals byte for byte.
    `out` must not share memory with src; returns out (include/stswin_hip.h, stswin_yuv_to_rgb)."""
    if fmt not in _YUV_FORMATS:
        raise StswinHipError(f"yuv_to_rgb: fmt must be one of {sorted(_YUV_FORMATS)}, got {fmt!r}")
    if chroma not in _YUV_CHROMA:
        raise StswinHipError(f"yuv_to_rgb: chroma must be one of {sorted(_YUV_CHROMA)}, got {chroma!r}")
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or not src.is_contiguous() or src.numel() == 0:
        raise StswinHipError("yuv_to_rgb: src must be a contiguous, non-empty uint8 tensor")
    if fmt == "nv12":
        if src.dim() != 3 or src.shape[1] % 3 or src.shape[2] % 2:
            raise StswinHipError(f"yuv_to_rgb: nv12 src must be uint8 [n][3 Hs / 2][Ws] with Hs and Ws even, got {tuple(src.shape)}")
        n, Hs, Ws = src.shape[0], src.shape[1] // 3 * 2, src.shape[2]
    else:
        if src.dim() != 4 or src.shape[3] != 2 or src.shape[2] % 2:
            raise StswinHipError(f"yuv_to_rgb: uyvy src must be uint8 [n][Hs][Ws][2] with Ws even, got {tuple(src.shape)}")
        n, Hs, Ws = src.shape[:3]
    _yuv_matrix(matrix, src.device, "yuv_to_rgb")
    if out is None:
        out = torch.empty(n, Hs, Ws, 3, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, Hs, Ws, 3) or not out.is_contiguous() or out.device != src.device:
        raise StswinHipError(f"yuv_to_rgb: out must be contiguous uint8 [{n}][{Hs}][{Ws}][3] on {src.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
    elif _same_memory(out, src) or _same_memory(out, matrix):
        raise StswinHipError("yuv_to_rgb: out shares memory with src or matrix")
    _check(load().stswin_yuv_to_rgb(_p(src), _p(matrix), _p(out), n, Hs, Ws, _YUV_FORMATS[fmt], _YUV_CHROMA[chroma], _stream()),
           "yuv_to_rgb")
    return out


def rgb_to_nv12(src: torch.Tensor, matrix: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB [n][Hs][Ws][3] (Hs, Ws even) -> NV12 uint8 [n][3 Hs / 2][Ws]: luma per pixel, chroma from the 2 x 2 block's mean, with
    matrix int32 [3][4] on the device (utils.yuv.to_yuv_matrix); equals utils.yuv.rgb_to_nv12 byte for byte.  `out` must not share
    memory with src; returns out (include/stswin_hip.h, stswin_rgb_to_nv12)."""
    if (not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or not src.is_contiguous()
            or src.numel() == 0 or src.shape[1] % 2 or src.shape[2] % 2):
        got = f"{src.dtype} {tuple(src.shape)}" if isinstance(src, torch.Tensor) else type(src).__name__
        raise StswinHipError(f"rgb_to_nv12: src must be contiguous, non-empty uint8 [n][Hs][Ws][3] with Hs and Ws even, got {got}")
    n, Hs, Ws, _ = src.shape
    _yuv_matrix(matrix, src.device, "rgb_to_nv12")
    if out is None:
        out = torch.empty(n, Hs // 2 * 3, Ws, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, Hs // 2 * 3, Ws) or not out.is_contiguous() or out.device != src.device:
        raise StswinHipError(f"rgb_to_nv12: out must be contiguous uint8 [{n}][{Hs // 2 * 3}][{Ws}] on {src.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
    elif _same_memory(out, src) or _same_memory(out, matrix):
        raise StswinHipError("rgb_to_nv12: out shares memory with src or matrix")
    _check(load().stswin_rgb_to_nv12(_p(src), _p(matrix), _p(out), n, Hs, Ws, _stream()), "rgb_to_nv12")
    return out


def _int_table(t: Optional[torch.Tensor], rows: int, what: str):
    if t is None:
        raise StswinHipError(f"frame_ingest: the {what} table is missing")
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != rows or not t.is_contiguous():
        raise StswinHipError(f"frame_ingest: the {what} table must be contiguous int32 [{rows}][k], got {t.dtype} {tuple(t.shape)}")
    return t


def frame_ingest(frames: torch.Tensor, out: torch.Tensor, lut: torch.Tensor, htab=None, vtab=None, tmp: Optional[torch.Tensor] = None):
    """uint8 HWC frames [n][Hs][Ws][3] -> fp32 NCHW images `out` [n][3][H][W], Pillow BILINEAR resize + the 256-entry value
    table `lut` (include/stswin_hip.h, stswin_frame_ingest), or with lut fp32 [3][256] one table per RGB plane
    (stswin_frame_ingest_planes).  htab / vtab = (bounds int32 [W|H][2], coef int32 [W|H][k]) for a width / height that changes;
    tmp = uint8 [n][Hs][W][3] when the width changes."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise StswinHipError(f"frame_ingest: frames must be contiguous uint8 [n][Hs][Ws][3], got {frames.dtype} {tuple(frames.shape)}")
    n, Hs, Ws, _ = frames.shape
    if out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[:2]) != (n, 3) or not out.is_contiguous():
        raise StswinHipError(f"frame_ingest: out must be contiguous fp32 [{n}][3][H][W], got {out.dtype} {tuple(out.shape)}")
    H, W = out.shape[2:]
    planes = lut.dim() == 2
    if lut.dtype != torch.float32 or not lut.is_contiguous() or tuple(lut.shape) not in ((256,), (3, 256)):
        raise StswinHipError(f"frame_ingest: lut must be contiguous fp32 [256] or [3][256], got {lut.dtype} {tuple(lut.shape)}")
    hb = hc = vb = vc = None
    hk = vk = 0
    if Ws != W:
        hb, hc = _int_table(htab[0] if htab else None, W, "horizontal bounds"), _int_table(htab[1] if htab else None, W, "horizontal weight")
        hk = hc.shape[1]
        if tmp is None or tmp.dtype != torch.uint8 or tmp.numel() < n * Hs * W * 3 or not tmp.is_contiguous():
            raise StswinHipError(f"frame_ingest: the width changes: tmp must be contiguous uint8 with >= {n * Hs * W * 3} bytes")
    if Hs != H:
        vb, vc = _int_table(vtab[0] if vtab else None, H, "vertical bounds"), _int_table(vtab[1] if vtab else None, H, "vertical weight")
        vk = vc.shape[1]
    entry = load().stswin_frame_ingest_planes if planes else load().stswin_frame_ingest
    _check(entry(_p(frames), _p(tmp if Ws != W else None), _p(out), n, Hs, Ws, H, W, _p(hb), _p(hc), hk, _p(vb), _p(vc), vk, _p(lut),
                 _stream()), "frame_ingest")
    return out


def clip_assemble(ring: torch.Tensor, fresh: Optional[torch.Tensor], clips: Optional[torch.Tensor], table: torch.Tensor, B: int,
                  n_store: int) -> None:
    """clips [B][4][...] <- ring [S][...] / fresh [n][...] frame features by `table` (int32 device [B*4 + n_store]: sources, then the
    ring slots fresh frames 0..n_store-1 go to); include/stswin_hip.h, stswin_clip_assemble.  The table's values are read on the
    device (a captured graph replays whatever the host last wrote into it)."""
    frame = ring[0].numel()
    for t, what in ((fresh, "fresh"), (clips, "clips")):
        if t is not None and (t.dtype != ring.dtype or not t.is_contiguous() or t.numel() % frame or t.device != ring.device):
            raise StswinHipError(f"clip_assemble: {what} must be contiguous {ring.dtype} frame features on {ring.device}")
    if not ring.is_contiguous():
        raise StswinHipError("clip_assemble: the ring must be contiguous")
    if table.dtype != torch.int32 or table.numel() < B * 4 + n_store or not table.is_contiguous():
        raise StswinHipError(f"clip_assemble: table must be contiguous int32 with >= {B * 4 + n_store} entries")
    n_fresh = fresh.numel() // frame if fresh is not None else 0
    if B > 0 and (clips is None or clips.numel() < B * 4 * frame):
        raise StswinHipError(f"clip_assemble: clips must hold {B} x 4 frames")
    if n_store > n_fresh:
        raise StswinHipError(f"clip_assemble: {n_store} stores but {n_fresh} fresh frames")
    _check(load().stswin_clip_assemble(_dt(ring), _p(ring), _p(fresh), _p(clips), _p(table), B, n_store, ring.shape[0], n_fresh,
                                       frame, _stream()), "clip_assemble")


def tensor_form(t, dtype, shape, what: str, fn: str, device=None) -> torch.Tensor:
    """t must be a contiguous GPU tensor of this dtype and shape (None in the shape: any extent)."""
    form = f"contiguous {str(dtype).replace('torch.', '')} [" + "][".join("n" if s is None else str(s) for s in shape) + "] on the GPU"
    if not isinstance(t, torch.Tensor):
        raise StswinHipError(f"{fn}: {what} must be a {form}, got {type(t).__name__}")
    ok = t.is_cuda and t.dtype == dtype and t.dim() == len(shape) and t.is_contiguous() and \
        all(s is None or s == d for s, d in zip(shape, t.shape)) and (device is None or t.device == device)
    if not ok:
        raise StswinHipError(f"{fn}: {what} must be a {form}, got {t.dtype} {tuple(t.shape)} on {t.device}"
                             + ("" if t.is_contiguous() else " (not contiguous)"))
    return t


def augment_crop_table_stride(Hc: int, Wc: int, ksize: int) -> int:
    return int(load().stswin_augment_crop_table_stride(Hc, Wc, ksize))


def augment_finish_table_stride(Hc: int, Wc: int) -> int:
    return int(load().stswin_augment_finish_table_stride(Hc, Wc))


def augment_crop(frames: torch.Tensor, labels: torch.Tensor, tmp: torch.Tensor, crop: torch.Tensor, label_crop: torch.Tensor,
                 table: torch.Tensor, ksize: int):
    """Stage 1 of the training transform: uint8 clips [B][T][Hs][Ws][3] and labels [B][Hs][Ws] -> uint8 crops `crop` [B][T][Hc][Wc][3]
    and `label_crop` [B][Hc][Wc], scaled (Pillow BILINEAR / NEAREST), padded, cropped and flipped by the per-sample int32 `table`
    [B][stride] (include/stswin_hip.h, stswin_augment_crop); tmp = uint8 with >= B*T*Hs*Wc*3 bytes."""
    fn = "augment_crop"
    tensor_form(frames, torch.uint8, (None, None, None, None, 3), "frames", fn)
    B, T, Hs, Ws, _ = frames.shape
    dev = frames.device
    tensor_form(labels, torch.uint8, (B, Hs, Ws), "labels", fn, dev)
    tensor_form(crop, torch.uint8, (B, T, None, None, 3), "crop", fn, dev)
    Hc, Wc = crop.shape[2:4]
    tensor_form(label_crop, torch.uint8, (B, Hc, Wc), "label_crop", fn, dev)
    tensor_form(table, torch.int32, (B, None), "table", fn, dev)
    if table.shape[1] < augment_crop_table_stride(Hc, Wc, ksize):
        raise StswinHipError(f"{fn}: table rows must hold >= {augment_crop_table_stride(Hc, Wc, ksize)} words, got {table.shape[1]}")
    if not isinstance(tmp, torch.Tensor) or not tmp.is_cuda or tmp.dtype != torch.uint8 or not tmp.is_contiguous() or \
            tmp.numel() < B * T * Hs * Wc * 3 or tmp.device != dev:
        raise StswinHipError(f"{fn}: tmp must be contiguous uint8 on the GPU with >= {B * T * Hs * Wc * 3} bytes")
    _check(load().stswin_augment_crop(_p(frames), _p(labels), _p(tmp), _p(crop), _p(label_crop), _p(table), table.shape[1], ksize, B, T,
                                      Hs, Ws, Hc, Wc, _stream()), fn)
    return crop, label_crop


def augment_finish(crop: torch.Tensor, label_crop: torch.Tensor, images: torch.Tensor, labels_out: torch.Tensor, table: torch.Tensor,
                   lut: torch.Tensor, label_lut: torch.Tensor):
    """Stage 2: uint8 crops [B][T][Hc][Wc][3] and label crops [B][Hc][Wc] -> fp32 `images` [B][T][3][Hc][Wc] and int64 `labels_out`
    [B][Hc][Wc]: the sample's value table, the fixed-point rotation, then lut (fp32 [256] or [3][256]) and label_lut (int64 [256]);
    per-sample int32 `table` [B][stride] (include/stswin_hip.h, stswin_augment_finish)."""
    fn = "augment_finish"
    tensor_form(crop, torch.uint8, (None, None, None, None, 3), "crop", fn)
    B, T, Hc, Wc, _ = crop.shape
    dev = crop.device
    tensor_form(label_crop, torch.uint8, (B, Hc, Wc), "label_crop", fn, dev)
    tensor_form(images, torch.float32, (B, T, 3, Hc, Wc), "images", fn, dev)
    tensor_form(labels_out, torch.int64, (B, Hc, Wc), "labels_out", fn, dev)
    tensor_form(table, torch.int32, (B, None), "table", fn, dev)
    if table.shape[1] < augment_finish_table_stride(Hc, Wc):
        raise StswinHipError(f"{fn}: table rows must hold >= {augment_finish_table_stride(Hc, Wc)} words, got {table.shape[1]}")
    tensor_form(lut, torch.float32, (3, 256) if isinstance(lut, torch.Tensor) and lut.dim() == 2 else (256,), "lut ([256] or [3][256])", fn, dev)
    tensor_form(label_lut, torch.int64, (256,), "label_lut", fn, dev)
    _check(load().stswin_augment_finish(_p(crop), _p(label_crop), _p(images), _p(labels_out), _p(table), table.shape[1], _p(lut),
                                        1 if lut.dim() == 2 else 0, _p(label_lut), B, T, Hc, Wc, _stream()), fn)
    return images, labels_out


def augment_noise(crop: torch.Tensor, table: torch.Tensor, thr: torch.Tensor, k_min: int):
    """CaDIS's Gaussian noise between the stages, in place: uint8 `crop` [B][...] (any trailing shape; a sample's bytes must be a
    multiple of 4), the stage-2 int32 `table` [B][stride] whose words 1 .. 3 hold (key low, key high, noise on), and the law as
    ascending thresholds `thr` (int32 holding the uint32 bit patterns, as torch has no uint32 arithmetic to offer; <= 1024 of them)
    with `k_min` (include/stswin_hip.h, stswin_augment_noise).  A sample with noise == 0 is not written."""
    fn = "augment_noise"
    if not isinstance(crop, torch.Tensor) or crop.dim() < 2:
        raise StswinHipError(f"{fn}: crop must be a contiguous uint8 [B][...] on the GPU, got {type(crop).__name__}"
                             + (f" {tuple(crop.shape)}" if isinstance(crop, torch.Tensor) else ""))
    tensor_form(crop, torch.uint8, (None,) * crop.dim(), "crop", fn)
    B, dev = crop.shape[0], crop.device
    sample_bytes = crop.numel() // B if B else 0
    if B == 0 or sample_bytes == 0 or sample_bytes % 4:
        raise StswinHipError(f"{fn}: a sample of crop must hold a positive multiple of 4 bytes, got {tuple(crop.shape)}")
    tensor_form(table, torch.int32, (B, None), "table", fn, dev)
    if table.shape[1] < augment_finish_table_stride(1, 1):
        raise StswinHipError(f"{fn}: table rows must hold >= {augment_finish_table_stride(1, 1)} words (stage 2's rows), got {table.shape[1]}")
    tensor_form(thr, torch.int32, (None,), "thr", fn, dev)
    if not 1 <= thr.shape[0] <= 1024:
        raise StswinHipError(f"{fn}: thr must hold 1 .. 1024 thresholds, got {thr.shape[0]}")
    _check(load().stswin_augment_noise(_p(crop), _p(table), table.shape[1], _p(thr), thr.shape[0], int(k_min), B, sample_bytes,
                                       _stream()), fn)
    return crop


def contrast_views_table_stride(H: int, W: int, ksize: int) -> int:
    return int(load().stswin_contrast_views_table_stride(H, W, ksize))


def contrast_views(frames: torch.Tensor, labels: torch.Tensor, tmp: torch.Tensor, images: torch.Tensor, masks: torch.Tensor,
                   table: torch.Tensor, lut: torch.Tensor, ksize: int):
    """The contrastive pre-training views: uint8 frames [F][Hs][Ws][3] and labels [L][Hs][Ws] -> fp32 `images` [V][4][3][H][W] and fp32
    `masks` [V][1][H][W], each view-sample cropped, resized (Pillow BILINEAR / NEAREST), flipped and converted through lut fp32
    [3][256] by its row of the int32 `table` [V][stride], which also names its four frames and its label (include/stswin_hip.h,
    stswin_contrast_views); tmp = uint8 with >= V*4*Hs*W*3 bytes.  The frame and label indices are the caller's to check (they live
    in device memory; the kernel clamps them)."""
    fn = "contrast_views"
    tensor_form(frames, torch.uint8, (None, None, None, 3), "frames", fn)
    F_, Hs, Ws, _ = frames.shape
    dev = frames.device
    tensor_form(labels, torch.uint8, (None, Hs, Ws), "labels", fn, dev)
    tensor_form(images, torch.float32, (None, 4, 3, None, None), "images", fn, dev)
    V, _, _, H, W = images.shape
    tensor_form(masks, torch.float32, (V, 1, H, W), "masks", fn, dev)
    tensor_form(table, torch.int32, (V, None), "table", fn, dev)
    if table.shape[1] < contrast_views_table_stride(H, W, ksize):
        raise StswinHipError(f"{fn}: table rows must hold >= {contrast_views_table_stride(H, W, ksize)} words, got {table.shape[1]}")
    tensor_form(lut, torch.float32, (3, 256), "lut", fn, dev)
    if not isinstance(tmp, torch.Tensor) or not tmp.is_cuda or tmp.dtype != torch.uint8 or not tmp.is_contiguous() or \
            tmp.numel() < V * 4 * Hs * W * 3 or tmp.device != dev:
        raise StswinHipError(f"{fn}: tmp must be contiguous uint8 on the GPU with >= {V * 4 * Hs * W * 3} bytes")
    _check(load().stswin_contrast_views(_p(frames), _p(labels), _p(tmp), _p(images), _p(masks), _p(table), table.shape[1], _p(lut), ksize,
                                        V, F_, labels.shape[0], Hs, Ws, H, W, _stream()), fn)
    return images, masks


def optim_tick(kind: int, counter: torch.Tensor, hyper: torch.Tensor, a: float, b: float) -> None:
    """Advance a device-resident step counter (int32 [1]) and derive the step's scalars into hyper (fp32 [4]); include/stswin_hip.h."""
    assert counter.dtype == torch.int32 and hyper.dtype == torch.float32 and hyper.numel() >= 4 and counter.is_cuda and hyper.is_cuda
    _check(load().stswin_optim_tick(int(kind), _p(counter), _p(hyper), a, b, _stream()), "optim_tick")


def _mt_lists(fn: str, ps, **lists) -> None:
    """The kernels read every list through raw pointers with the parameters' element counts: each tensor must be contiguous fp32 on
    the parameters' GPU and as long as its parameter (checked before any launch)."""
    dev = ps[0].device if len(ps) else None
    f32 = torch.float32
    for name, ts in (("ps", ps), *lists.items()):
        if ts is None:
            continue
        if len(ts) != len(ps):
            raise StswinHipError(f"{fn}: {name} holds {len(ts)} tensors for {len(ps)} parameters")
        for i, (t, p) in enumerate(zip(ts, ps)):
            if not (t.is_cuda and t.device == dev and t.dtype == f32 and t.is_contiguous() and t.numel() == p.numel()):
                raise StswinHipError(f"{fn}: {name}[{i}] must be a contiguous float32 tensor of {p.numel()} elements on {dev}, got "
                                     f"{t.dtype} {tuple(t.shape)} on {t.device}" + ("" if t.is_contiguous() else " (not contiguous)"))


def multi_tensor(mode, ps, gs, ms=None, vs=None, lr=0.0, b1=0.0, b2=0.0, eps=0.0, wd=0.0, c1=1.0, c2=1.0, hyper=None):
    """mode 0 Adam / 1 SGD-momentum / 2 EMA over lists of fp32 tensors (chunks of 48 tensors per launch).  hyper (device fp32 [4] =
    {lr, c1, c2, EMA momentum}): read the step-dependent scalars from it instead of lr / c1 / c2 / b1(EMA) - for SGD c1 != 0 still
    marks the first step."""
    lib = load()
    st = _stream()
    _mt_lists("multi_tensor", ps, gs=gs, ms=ms, vs=vs)
    for lo in range(0, len(ps), 48):
        hi = min(len(ps), lo + 48)
        k = hi - lo
        arr = lambda ts: (_c_void_p * k)(*[t.data_ptr() for t in ts[lo:hi]]) if ts is not None else None  # noqa: E731
        ns = (_c_int * k)(*[t.numel() for t in ps[lo:hi]])
        if hyper is not None:
            _check(lib.stswin_multi_tensor_dev(mode, k, arr(ps), arr(gs), arr(ms), arr(vs), ns, _p(hyper), b1, b2,
                                               eps, wd, 1 if (mode == 1 and c1 != 0.0) else 0, st), "multi_tensor_dev")
        else:
            _check(lib.stswin_multi_tensor(mode, k, arr(ps), arr(gs), arr(ms), arr(vs), ns, lr, b1,
                                           b2, eps, wd, c1, c2, st),
                   "multi_tensor")


def multi_tensor_lars(ps, gs, ms, norms, *, lr, momentum, wd, trust_coef, eps, first, adaptive, hyper=None):
    """LARS-scaled SGD-momentum step of one parameter group (lists of contiguous fp32 GPU tensors; chunks of 48 tensors,
    three launches each: partial norms, their fold, update).  norms: None, or fp32 scratch that every 48-tensor launch uses in turn
    when it holds that launch's 2 * tensors + 2 * sum ceil(n / 8192) floats (the launch's [tensors][2] norms come first); a launch
    that needs more takes the library's scratch instead."""
    lib = load()
    st = _stream()
    _mt_lists("multi_tensor_lars", ps, gs=gs, ms=ms)
    if norms is not None and not (norms.is_cuda and norms.dtype == torch.float32 and norms.is_contiguous()
                                  and (not len(ps) or norms.device == ps[0].device)):
        raise StswinHipError("multi_tensor_lars: norms must be a contiguous float32 tensor on the parameters' GPU")
    for lo in range(0, len(ps), 48):
        hi = min(len(ps), lo + 48)
        k = hi - lo
        arr = lambda ts: (_c_void_p * k)(*[t.data_ptr() for t in ts[lo:hi]])  # noqa: E731
        ns = (_c_int * k)(*[t.numel() for t in ps[lo:hi]])
        need = 2 * k + 2 * sum((t.numel() + 8191) // 8192 for t in ps[lo:hi])
        if norms is None or norms.numel() < need:
            norms = scratch(ps[lo].device, need)
        if hyper is not None:          # the learning rate from device memory (hyper[0])
            _check(lib.stswin_multi_tensor_lars_dev(k, arr(ps), arr(gs), arr(ms), ns, _p(norms), norms.numel(), _p(hyper),
                                                    momentum, wd, trust_coef, eps, 1 if first else 0,
                                                    1 if adaptive else 0, st), "multi_tensor_lars_dev")
            continue
        _check(lib.stswin_multi_tensor_lars(k, arr(ps), arr(gs), arr(ms), ns, _p(norms), norms.numel(), lr, momentum,
                                            wd, trust_coef, eps, 1 if first else 0,
                                            1 if adaptive else 0, st), "multi_tensor_lars")


def proxy_collective(src: torch.Tensor, dst: torch.Tensor, workgroups: int, passes: int) -> None:
    """Measurement stand-in for an RCCL all-reduce of a bucket (include/stswin_hip.h; tools/overlap_proxy.py): `workgroups` workgroups hold
    their compute units while they copy src -> dst `passes` times, on the current stream."""
    assert src.numel() * src.element_size() == dst.numel() * dst.element_size() and src.is_contiguous() and dst.is_contiguous()
    _check(load().stswin_proxy_collective(_p(src), _p(dst), src.numel() * src.element_size(), workgroups, passes, _stream()),
           "proxy_collective")


def set_cu_budget(cus: int) -> int:
    """Compute units the one-workgroup-per-CU launches plan for (0 = the whole device); returns the previous setting."""
    return int(load().stswin_set_cu_budget(int(cus)))


def calibrate(device=None, seconds: float = 0.1) -> dict:
    """Box calibration for bench lines (include/stswin_hip.h: stswin_calib_mfma / stswin_calib_copy): sustained bf16 MFMA TFLOP/s of a
    register-only loop (4 waves per CU) and sustained copy TB/s (read + write) over 2 x 512 MB, each the best of three timed launches
    of ~`seconds`/3 after a warm-up launch.  HIP events on the current stream."""
    lib = load()
    dev = torch.device(device if device is not None else "cuda")
    sink = torch.zeros(4, dtype=torch.float32, device=dev)
    st = _stream()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    iters = int(300000 * max(seconds, 0.01) / 0.1)
    per = int(lib.stswin_calib_mfma(4, 20000, _p(sink), st))                      # warm-up
    t = min(timed(lambda: lib.stswin_calib_mfma(4, iters, _p(sink), st)) for _ in range(3))
    tflops = per * iters * 16384.0 / t / 1e12
    n = 512 << 20
    src = torch.empty(n, dtype=torch.uint8, device=dev)
    dst = torch.empty(n, dtype=torch.uint8, device=dev)
    src.zero_()
    _check(lib.stswin_calib_copy(_p(src), _p(dst), n, st), "calib_copy")
    tc = min(timed(lambda: lib.stswin_calib_copy(_p(src), _p(dst), n, st)) for _ in range(3))
    del src, dst
    return {"mfma_bf16_tflops": tflops, "mfma_probe_ms": t * 1e3, "copy_tbps": 2.0 * n / tc / 1e12, "copy_probe_ms": tc * 1e3}


def selftest(which: int) -> torch.Tensor:
    out = torch.zeros(16384, dtype=torch.float32, device="cuda")
    if which == 5:
        out[:512] = torch.arange(512, dtype=torch.float32, device="cuda")
    _check(load().stswin_selftest(_p(out), which, _stream()), "selftest")
    torch.cuda.synchronize()
    return out.cpu()
