"""Float64 reference of the window-attention core (swin_512.py:117-138) in the call forms of the library's kernels.

Shared by tests/test_attn_ref.py (CPU: the reference against the oracle, autograd and the older private helpers) and
tests/test_hip_attention_contract.py (GPU: every attention kernel against it).  Nothing here calls the library: it is plain torch,
run on whatever device its inputs live on (the GPU tests keep it there in float64, so production window counts stay cheap).

Layouts are the kernels' (include/stswin_hip.h, a6 section):
  qkv   [nB_ * T * N][3C]   q (pre-scaled by d^-0.5) | k | v, rows in window order (window b_, frame t, position n)
  bias  one of the three `bias_windows` forms, all [key n][query n] (transposed):
          "1"  : biasT [heads][N][N], optional maskT [nW][N][N] added per window
          "nW" : biasT [nW][heads][N][N] = bias + mask already summed, no index
          "U"  : biasT [U][heads][N][N] and bias_index [nW] (window w reads slot bias_index[w])
        window b_ uses entry b_ % nW; the [N][N] tables repeat over the T x T frame blocks of a window.
  dbiasT [heads][N][N] [key][query]: the gradient of the per-head bias, summed over windows and frame blocks.
"""
from __future__ import annotations

import torch

F64 = torch.float64


def window_bias(biasT, maskT=None, *, nW, bias_index=None):
    """Any of the three forms -> the bias + mask every window of the pattern sees, [nW][heads][N][N] float64, [query][key]
    (the one place where the kernels' transposed layout is undone)."""
    b = biasT.to(F64)
    if b.dim() == 3:                                           # "1": one per-head table, the mask added per window
        w = b.unsqueeze(0).expand(nW, *b.shape)
        if maskT is not None:
            assert maskT.shape[0] == nW
            w = w + maskT.to(F64).unsqueeze(1)
    else:
        assert maskT is None, "the pre-summed forms carry the mask in the table"
        if bias_index is None:                                 # "nW": one table per window
            assert b.shape[0] == nW
            w = b
        else:                                                  # "U": slot table + window -> slot index
            idx = bias_index.to(device=b.device, dtype=torch.long)
            assert idx.shape == (nW,) and int(idx.min()) >= 0 and int(idx.max()) < b.shape[0]
            w = b[idx]
    return w.transpose(-1, -2)


def _split(qkv, nB_, T, N, heads, C):
    d = C // heads
    x = qkv.to(F64).reshape(nB_, T * N, 3, heads, d).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]                                    # each [nB_][heads][T N][d]


def _merge(x, nB_, T, N, C):
    return x.transpose(1, 2).reshape(nB_ * T * N, C)


def scores(qkv, biasT, maskT=None, *, T, ws, heads, C, nW, bias_index=None):
    """S = q_s k^T + bias (+ mask), both tiled over the T x T frame blocks: [nB_][heads][T N][T N] float64."""
    N = ws * ws
    nB_ = qkv.shape[0] // (T * N)
    assert nB_ * T * N == qkv.shape[0] and nB_ % nW == 0 and qkv.shape[1] >= 3 * C
    q, k, _ = _split(qkv[:, :3 * C], nB_, T, N, heads, C)
    bw = window_bias(biasT, maskT, nW=nW, bias_index=bias_index).to(q.device).repeat(1, 1, T, T)    # [nW][heads][TN][TN]
    s = (q @ k.transpose(-1, -2)).reshape(nB_ // nW, nW, heads, T * N, T * N) + bw.unsqueeze(0)
    return s.reshape(nB_, heads, T * N, T * N)


def attention(qkv, biasT, maskT=None, *, T, ws, heads, C, nW, bias_index=None, dout=None, scale=1.0):
    """The forward and, with dout, the backward of the attention core, in float64 on qkv's device.

    Returns a dict: out [rows][C]; with dout also dq (= scale * dL/dq_s, as the kernels write it), dk, dv [rows][C], dqkv
    [rows][3C] (dq | dk | dv), dbiasT [heads][N][N] ([key][query], summed over windows and frame blocks) and colsum [C] (column
    sums of dq, the q third of the qkv-bias gradient).  The backward is written out (dS = P o (dP - rowsum(P o dP))); the CPU
    tests hold it against float64 autograd."""
    N = ws * ws
    nB_ = qkv.shape[0] // (T * N)
    s = scores(qkv, biasT, maskT, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bias_index)
    p = torch.softmax(s, dim=-1)
    q, k, v = _split(qkv[:, :3 * C], nB_, T, N, heads, C)
    res = {"out": _merge(p @ v, nB_, T, N, C), "p": p}
    if dout is None:
        return res
    do = dout.to(F64).reshape(nB_, T * N, heads, C // heads).transpose(1, 2)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dq = _merge(ds @ k, nB_, T, N, C) * scale
    dk = _merge(ds.transpose(-1, -2) @ q, nB_, T, N, C)
    dv = _merge(p.transpose(-1, -2) @ do, nB_, T, N, C)
    db = ds.sum(0).reshape(heads, T, N, T, N).sum((1, 3))     # [heads][query n][key n]
    res.update(dq=dq, dk=dk, dv=dv, dqkv=torch.cat([dq, dk, dv], 1), dbiasT=db.transpose(1, 2).contiguous(), colsum=dq.sum(0))
    return res


def e4m3_quantise(x, rows_per_problem, head_dim):
    """[rows][cols] -> (uint8 OCP e4m3 bytes, fp32 scales [rows / rows_per_problem][cols / head_dim]) with one amax / 448 scale per
    (problem, head column block): the storage format of stswin_gemm_nt_qkv_fp8, computed here from given values (fp32 arithmetic,
    round to nearest even), so that a test can hand the fp8 kernels operands of its own choosing."""
    rows, cols = x.shape
    xf = x.float()
    blk = xf.reshape(rows // rows_per_problem, rows_per_problem, cols // head_dim, head_dim)
    amax = blk.abs().amax(dim=(1, 3))
    sc = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    full = sc.repeat_interleave(rows_per_problem, 0).repeat_interleave(head_dim, 1)
    q8 = (xf / full).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q8.view(torch.uint8), sc


def e4m3_dequantise(q8, scales, rows_per_problem, head_dim):
    """uint8 e4m3 bytes + per-(problem, head block) scales -> float64 values (byte value x scale)."""
    v = q8.view(torch.float8_e4m3fn).to(F64)
    return v * scales.to(F64).repeat_interleave(rows_per_problem, 0).repeat_interleave(head_dim, 1)


def errors(got, ref):
    """(max |got - ref| / max |ref|, ||got - ref|| / ||ref||), float64 on ref's device."""
    g = got.to(device=ref.device, dtype=F64)
    r = ref.to(F64)
    den = float(r.abs().max())
    diff = g - r
    return float(diff.abs().max()) / max(den, 1e-300), float(diff.norm() / r.norm().clamp_min(1e-300))
