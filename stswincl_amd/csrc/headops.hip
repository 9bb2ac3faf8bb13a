// Decode-head and loss kernels on NHWC "token" matrices [M = frames*H*W rows][C channels] (HBM-bound work;
// 16-byte pieces per lane everywhere).  BatchNorm is grouped: the M rows are G equal groups with separate batch
// statistics (G = 1 for the head; G = frames lets the per-frame ResNet calls of base18.py:86-89 be batched without
// changing the per-frame statistics the reference computes).
#include "common.h"
#include <cstdlib>

// ----------------------------------------------------------------------------------------- column statistics
// sum[g][c] += sum_rows (x - pivot), sumsq[g][c] += sum_rows (x - pivot)^2, pivot = x[first row of group][c]
// (shifted sums keep E[x^2]-E[x]^2 well conditioned).  Block = 32 column pieces x 8 row lanes.
// Thread layout of the column-reduction / column-owner kernels: `cpb` column pieces (16 B each) x `256/cpb` row lanes,
// cpb = min(32, C/PACK) rounded down to a power of two, so narrow matrices (C = 64) still use every thread.
// rows per block for the column-reduction kernels: as many as possible (the LDS fold and the atomics are per block)
// while still launching >= ~1024 blocks
static int reduce_rows_per_chunk(int group_rows, int other_blocks, int nrl) {
  int rpc = 8 * nrl;
  while (rpc < 64 * nrl && (long)other_blocks * ((group_rows + 2 * rpc - 1) / (2 * rpc)) >= 1024) rpc *= 2;
  return rpc;
}
// Rows per thread of the BatchNorm backward passes: as many as leave about 512 (reduce pass: the LDS fold and the slab are per
// workgroup) or 2048 (dx pass) workgroups.  Until round 5 the dx pass ran 512, too: every thread loaded its 8 channels' constants
// from six arrays (48 loads + the arithmetic in front of the first row - a quarter of the pass, and the reason why smaller
// workgroups were slower); now one thread per channel computes them and LDS hands them out, and the dx pass is 25-30 % faster at
// 2048 workgroups (layer5: 63 -> 43 us, stem: 96 -> 79 us on cold operands; profiles/r05_bn_dx_prologue_experiment.txt,
// r05_bn_bwd_lds_constants_sweep.txt; step +1.1 % same box).
static int bn_bwd_rows(long rows_all_groups, int col_blocks, int nrl, int max_rows) {
  // (workgroup target: STSWIN_BN_RED_WGS for the reduce pass [max_rows 64], STSWIN_BN_DX_WGS for the dx pass [max_rows 32]; tuning knobs, read once)
  static const int tgt_red = getenv("STSWIN_BN_RED_WGS") ? atoi(getenv("STSWIN_BN_RED_WGS")) : 512;
  static const int tgt_dx = getenv("STSWIN_BN_DX_WGS") ? atoi(getenv("STSWIN_BN_DX_WGS")) : 2048;
  const int tgt = max_rows > 32 ? tgt_red : tgt_dx;
  int rows = 8;
  while (rows < max_rows && (long)col_blocks * (rows_all_groups / ((long)2 * rows * nrl)) >= tgt) rows *= 2;
  return rows;
}

// First physical row of the rows a block works on, minus its first row index inside the group: contiguous groups
// (unit == 0) start at g * group_rows; interleaved groups (unit > 0: group g owns the units g, g + G, g + 2G, ... of `unit`
// rows - frame t of every clip when the batch is stored clip-major) map the chunk's unit; a chunk never straddles a unit
// (the launchers make rows_per_chunk divide unit).
DEVI long group_row0(int g, int ch, int rows_per_chunk, int group_rows, int unit, int G) {
  if (unit <= 0) return (long)g * group_rows;
  return ((long)((ch * rows_per_chunk) / unit) * (G - 1) + g) * unit;
}
DEVI long group_first_row(int g, int group_rows, int unit) { return unit > 0 ? (long)g * unit : (long)g * group_rows; }
static int fit_chunk(int rpc, int unit) {            // largest power-of-two shrink of rpc that divides unit; 0: impossible
  if (unit <= 0) return rpc;
  while (rpc > 1 && unit % rpc) rpc >>= 1;
  return unit % rpc ? 0 : rpc;
}

static int pick_cpb(int pieces_per_row) {
  int c = 32;
  while (c > pieces_per_row) c >>= 1;
  return c < 1 ? 1 : c;
}

template <typename T, bool SQ>
__global__ __launch_bounds__(256) void colstats_kernel(const T* x, long ldx, float* part, int C, int group_rows,
                                                        int chunks_per_group, int rows_per_chunk, int cpb, int unit) {
  constexpr int PACK = TT<T>::PACK;
  __shared__ float lpart[2][256 * 8];
  const int cp = threadIdx.x % cpb, rl = threadIdx.x / cpb, nrl = 256 / cpb;
  const int c = (blockIdx.x * cpb + cp) * PACK;
  const int g = blockIdx.y / chunks_per_group, ch = blockIdx.y % chunks_per_group;
  const long gr0 = group_row0(g, ch, rows_per_chunk, group_rows, unit, gridDim.y / chunks_per_group);
  float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c < C) {
    if (SQ) {
      Vec16<T> p0;
      p0.v = *(const decltype(p0.v)*)(x + group_first_row(g, group_rows, unit) * ldx + c);
#pragma unroll
      for (int e = 0; e < PACK; ++e) pv[e] = p0.get(e);
    }
    const int r_end = min(group_rows, (ch + 1) * rows_per_chunk);
    for (int r = ch * rows_per_chunk + rl; r < r_end; r += nrl) {
      Vec16<T> in;
      in.v = *(const decltype(in.v)*)(x + (gr0 + r) * ldx + c);
#pragma unroll
      for (int e = 0; e < PACK; ++e) {
        const float d = in.get(e) - pv[e];
        a1[e] += d;
        if (SQ) a2[e] += d * d;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { lpart[0][(rl * cpb + cp) * 8 + e] = a1[e]; lpart[1][(rl * cpb + cp) * 8 + e] = a2[e]; }
  __syncthreads();
  {   // parallel fold: thread t < cpb*8 owns (column piece t/8, element t%8) and adds the nrl row-lane partials
    const int t = threadIdx.x, fc = t >> 3, fe = t & 7;
    const int cc = (blockIdx.x * cpb + fc) * PACK + fe;
    if (fc < cpb && fe < PACK && cc < C) {
      float s1 = 0.f, s2 = 0.f;
      for (int k = 0; k < nrl; ++k) { s1 += lpart[0][(k * cpb + fc) * 8 + fe]; s2 += lpart[1][(k * cpb + fc) * 8 + fe]; }
      // slab blockIdx.y = (group, row chunk) of the caller's scratch: [2][C] (plain stores; slab_fold_kernel adds the chunks of a
      // group in order: deterministic statistics, no same-address atomics)
      float* slab = part + (long)blockIdx.y * 2 * C;
      slab[cc] = s1;
      if (SQ) slab[C + cc] = s2;
    }
  }
}

// mean/rstd per (group, channel) from the shifted sums; running-stat update group by group in order
// (nn.BatchNorm2d momentum semantics: running = (1-m) running + m stat, unbiased variance).
template <typename T>
__global__ void bn_finalize_kernel(const T* x, long ldx, const float* sum, const float* sumsq, float* mean, float* rstd,
                                   float* running_mean, float* running_var, int C, int G, int group_rows, float eps,
                                   float momentum, int unit) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float rm = running_mean ? running_mean[c] : 0.f, rv = running_var ? running_var[c] : 0.f;
  for (int g = 0; g < G; ++g) {
    const float pivot = x ? to_f32<T>(x[group_first_row(g, group_rows, unit) * ldx + c]) : 0.f;   // (sums from a GEMM epilogue: raw)
    const float ms = sum[(long)g * C + c] / group_rows;
    const float var = fmaxf(sumsq[(long)g * C + c] / group_rows - ms * ms, 0.f);
    mean[(long)g * C + c] = pivot + ms;
    rstd[(long)g * C + c] = rsqrtf(var + eps);
    rm = (1.f - momentum) * rm + momentum * (pivot + ms);
    rv = (1.f - momentum) * rv + momentum * var * ((float)group_rows / (float)max(group_rows - 1, 1));
  }
  if (running_mean) { running_mean[c] = rm; running_var[c] = rv; }
}

// y = act( (x-mean)*rstd*gamma + beta [+ resid] ).  A thread owns one 16-byte channel piece and walks rows (stride 8
// inside its row chunk), so the per-channel scale/shift live in registers instead of being re-loaded per piece.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* x, long ldx, const float* mean, const float* rstd,
                                                        const float* gamma, const float* beta, const T* resid, long ldr,
                                                        T* y, long ldy, int C, int group_rows, int chunks_per_group,
                                                        int rows_per_chunk, int relu, int cpb, int unit) {
  constexpr int PACK = TT<T>::PACK;
  __shared__ __attribute__((aligned(16))) float coef[2][256];
  const int cp = threadIdx.x % cpb, rl = threadIdx.x / cpb, nrl = 256 / cpb;
  const int c = (blockIdx.x * cpb + cp) * PACK;
  const int g = blockIdx.y / chunks_per_group, ch = blockIdx.y % chunks_per_group;
  const long gr0 = group_row0(g, ch, rows_per_chunk, group_rows, unit, gridDim.y / chunks_per_group);
  {   // scale / shift of the workgroup's cpb * PACK <= 256 channels: one thread per channel, handed out through LDS (bn_bwd_dx_kernel)
    const int t = threadIdx.x, cc = blockIdx.x * cpb * PACK + t;
    if (t < cpb * PACK && cc < C) {
      const float rs = rstd[(long)g * C + cc] * gamma[cc];
      coef[0][t] = rs;
      coef[1][t] = beta[cc] - mean[(long)g * C + cc] * rs;
    }
  }
  __syncthreads();
  if (c >= C) return;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < PACK; e += 4) {
    *(f32x4*)(sc + e) = *(const f32x4*)&coef[0][cp * PACK + e];
    *(f32x4*)(sh + e) = *(const f32x4*)&coef[1][cp * PACK + e];
  }
  const int r_end = min(group_rows, (ch + 1) * rows_per_chunk);
  for (int r = ch * rows_per_chunk + rl; r < r_end; r += nrl) {
    Vec16<T> in, rs, o;
    in.v = *(const decltype(in.v)*)(x + (gr0 + r) * ldx + c);
    if (resid) rs.v = *(const decltype(rs.v)*)(resid + (gr0 + r) * ldr + c);
#pragma unroll
    for (int e = 0; e < PACK; ++e) {
      float v = in.get(e) * sc[e] + sh[e];
      if (resid) v += rs.get(e);
      if (relu) v = fmaxf(v, 0.f);
      o.set(e, v);
    }
    *(decltype(o.v)*)(y + (gr0 + r) * ldy + c) = o.v;
  }
}

// pass 1 of the backward: s1[g][c] = sum dyr, s2[g][c] = sum dyr*xhat, dyr = dy * (y > 0 if relu)
// Both passes walk their rows four at a time with all loads of the four rows issued first (one row per iteration left a
// thread with 2-3 requests in flight: 2.0-3.6 TB/s against the 5.4-6.5 TB/s of bn_apply, tools/bench_bn.py).
// ReLU mask: from the stored output y, or - when there is no residual, y == NULL - recomputed from x with bn_apply's own
// expression x * (rstd*gamma) + (beta - mean*rstd*gamma) > 0 (the same operations in the same order: the same sign): one
// tensor less to read in both passes.
#ifndef BN_BWD_U
#define BN_BWD_U 4
#endif
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* dy, long lddy, const T* x, long ldx, const T* y, long ldy,
                                                             const float* mean, const float* rstd, float* spart,
                                                             int C, int group_rows, int chunks_per_group, int rows_per_chunk,
                                                             int relu, int cpb, const float* gamma, const float* beta, int unit) {
  constexpr int PACK = TT<T>::PACK;
  constexpr int U = BN_BWD_U;
  __shared__ __attribute__((aligned(16))) float part[2][256 * 8];
  const int cp = threadIdx.x % cpb, rl = threadIdx.x / cpb, nrl = 256 / cpb;
  const int c = (blockIdx.x * cpb + cp) * PACK;
  const int g = blockIdx.y / chunks_per_group, ch = blockIdx.y % chunks_per_group;
  const long gr0 = group_row0(g, ch, rows_per_chunk, group_rows, unit, gridDim.y / chunks_per_group);
  float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool remask = relu && y == nullptr, ymask = relu && y != nullptr;
  {   // channel constants: one thread per channel, handed out through LDS (see bn_bwd_dx_kernel); `part` is free until the fold
    const int t = threadIdx.x, cc = blockIdx.x * cpb * PACK + t;
    if (t < cpb * PACK && cc < C) {
      const float m = mean[(long)g * C + cc], r = rstd[(long)g * C + cc];
      const float pmv = remask ? r * gamma[cc] : 0.f;
      part[0][t] = m; part[0][256 + t] = r; part[0][512 + t] = pmv; part[0][768 + t] = remask ? beta[cc] - m * pmv : 0.f;
    }
  }
  __syncthreads();
  float mu[8], rs[8], pm[8], qm[8];
  if (c < C) {
#pragma unroll
    for (int e = 0; e < PACK; e += 4) {
      *(f32x4*)(mu + e) = *(const f32x4*)&part[0][cp * PACK + e];
      *(f32x4*)(rs + e) = *(const f32x4*)&part[0][256 + cp * PACK + e];
      *(f32x4*)(pm + e) = *(const f32x4*)&part[0][512 + cp * PACK + e];
      *(f32x4*)(qm + e) = *(const f32x4*)&part[0][768 + cp * PACK + e];
    }
  }
  __syncthreads();
  if (c < C) {
    const int r_end = min(group_rows, (ch + 1) * rows_per_chunk);
    for (int r = ch * rows_per_chunk + rl; r < r_end; r += U * nrl) {
      Vec16<T> d[U], xi[U], yo[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (r + u * nrl < r_end) {
          const long row = gr0 + r + u * nrl;
          d[u].v = *(const decltype(d[u].v)*)(dy + row * lddy + c);
          xi[u].v = *(const decltype(xi[u].v)*)(x + row * ldx + c);
          if (ymask) yo[u].v = *(const decltype(yo[u].v)*)(y + row * ldy + c);
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (r + u * nrl < r_end) {
#pragma unroll
          for (int e = 0; e < PACK; ++e) {
            float dv = d[u].get(e);
            const float xv = xi[u].get(e);
            if (remask) { if (!(xv * pm[e] + qm[e] > 0.f)) dv = 0.f; }
            else if (ymask) { if (!(yo[u].get(e) > 0.f)) dv = 0.f; }
            a1[e] += dv;
            a2[e] += dv * ((xv - mu[e]) * rs[e]);
          }
        }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { part[0][(rl * cpb + cp) * 8 + e] = a1[e]; part[1][(rl * cpb + cp) * 8 + e] = a2[e]; }
  __syncthreads();
  {
    const int t = threadIdx.x, fc = t >> 3, fe = t & 7;
    const int cc = (blockIdx.x * cpb + fc) * PACK + fe;
    if (fc < cpb && fe < PACK && cc < C) {
      float t1 = 0.f, t2 = 0.f;
      for (int k = 0; k < nrl; ++k) { t1 += part[0][(k * cpb + fc) * 8 + fe]; t2 += part[1][(k * cpb + fc) * 8 + fe]; }
      float* slab = spart + (long)blockIdx.y * 2 * C;          // [(group, chunk)][2][C]: summed per group by slab_fold_kernel
      slab[cc] = t1;
      slab[C + cc] = t2;
    }
  }
}

// pass 2: dx = gamma*rstd*(dyr - [training] (s1 + xhat*s2)/n) ; dresid = dyr (optional).  Column-owner threads.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const T* dy, long lddy, const T* x, long ldx, const T* y, long ldy,
                                                         const float* mean, const float* rstd, const float* gamma,
                                                         const float* s1, const float* s2, T* dx, long lddx, T* dres,
                                                         long lddr, int C, int group_rows, int chunks_per_group,
                                                         int rows_per_chunk, int relu, int training, int cpb, float inv_n,
                                                         const float* beta, int unit, float* gsum) {
  constexpr int PACK = TT<T>::PACK;
  constexpr int U = BN_BWD_U;
  __shared__ __attribute__((aligned(16))) float coef[5][256];
  const int cp = threadIdx.x % cpb, rl = threadIdx.x / cpb, nrl = 256 / cpb;
  const int c = (blockIdx.x * cpb + cp) * PACK;
  const int g = blockIdx.y / chunks_per_group, ch = blockIdx.y % chunks_per_group;
  const long gr0 = group_row0(g, ch, rows_per_chunk, group_rows, unit, gridDim.y / chunks_per_group);
  const bool remask = relu && y == nullptr, ymask = relu && y != nullptr;
  // dx = A*dyr + B*x + D  with  A = gamma*rstd, B = -A*rstd*s2/n, D = -A*s1/n - B*mean      (training)
  // The workgroup's cpb * PACK <= 256 channels get their five constants from ONE thread each (coalesced loads) and LDS hands every
  // thread its 8: as 48 per-thread loads + the arithmetic in front of the first row the prologue was a quarter of the pass and
  // made more, smaller workgroups slower (profiles/r05_bn_dx_prologue_experiment.txt).
  {
    const int t = threadIdx.x, cc = blockIdx.x * cpb * PACK + t;
    if (t < cpb * PACK && cc < C) {
      const long gc = (long)g * C + cc;
      const float rsd = rstd[gc], mu = mean[gc], ga = gamma[cc];
      const float A = ga * rsd;
      const float kbv = training ? -A * rsd * s2[gc] * inv_n : 0.f;
      const float pmv = remask ? rsd * ga : 0.f;
      coef[0][t] = A;
      coef[1][t] = kbv;
      coef[2][t] = training ? -A * s1[gc] * inv_n - kbv * mu : 0.f;
      coef[3][t] = pmv;
      coef[4][t] = remask ? beta[cc] - mu * pmv : 0.f;
    }
  }
  __syncthreads();
  if (c >= C) return;
  if (gsum && blockIdx.y == 0 && rl == 0) {              // parameter gradients: dbeta | dgamma = s1 | s2 summed over the groups
    const int G = gridDim.y / chunks_per_group;
#pragma unroll
    for (int e = 0; e < PACK; ++e) {
      float a = 0.f, b = 0.f;
      for (int gg = 0; gg < G; ++gg) { a += s1[(long)gg * C + c + e]; b += s2[(long)gg * C + c + e]; }
      gsum[c + e] = a;
      gsum[C + c + e] = b;
    }
  }
  float ka[8], kb[8], kd[8], pm[8], qm[8];
#pragma unroll
  for (int e = 0; e < PACK; e += 4) {
    *(f32x4*)(ka + e) = *(const f32x4*)&coef[0][cp * PACK + e];
    *(f32x4*)(kb + e) = *(const f32x4*)&coef[1][cp * PACK + e];
    *(f32x4*)(kd + e) = *(const f32x4*)&coef[2][cp * PACK + e];
    *(f32x4*)(pm + e) = *(const f32x4*)&coef[3][cp * PACK + e];
    *(f32x4*)(qm + e) = *(const f32x4*)&coef[4][cp * PACK + e];
  }
  const int r_end = min(group_rows, (ch + 1) * rows_per_chunk);
  for (int r = ch * rows_per_chunk + rl; r < r_end; r += U * nrl) {
    Vec16<T> d[U], xi[U], yo[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (r + u * nrl < r_end) {
        const long row = gr0 + r + u * nrl;
        d[u].v = *(const decltype(d[u].v)*)(dy + row * lddy + c);
        xi[u].v = *(const decltype(xi[u].v)*)(x + row * ldx + c);
        if (ymask) yo[u].v = *(const decltype(yo[u].v)*)(y + row * ldy + c);
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (r + u * nrl < r_end) {
        const long row = gr0 + r + u * nrl;
        Vec16<T> o, od;
#pragma unroll
        for (int e = 0; e < PACK; ++e) {
          float dv = d[u].get(e);
          const float xv = xi[u].get(e);
          if (remask) { if (!(xv * pm[e] + qm[e] > 0.f)) dv = 0.f; }
          else if (ymask) { if (!(yo[u].get(e) > 0.f)) dv = 0.f; }
          o.set(e, ka[e] * dv + kb[e] * xv + kd[e]);
          od.set(e, dv);
        }
        *(decltype(o.v)*)(dx + row * lddx + c) = o.v;
        if (dres) *(decltype(od.v)*)(dres + row * lddr + c) = od.v;
      }
  }
}

// out[r][c] (+)= v[r / group_rows][c] * scale      (image-pool broadcast and adaptive-avg-pool backward)
template <typename T>
__global__ __launch_bounds__(256) void rows_broadcast_kernel(const float* v, T* out, long ldo, int M, int C, int group_rows,
                                                              float scale, int accumulate) {
  constexpr int PACK = TT<T>::PACK;
  const int ppr = C / PACK;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * ppr) return;
  const int r = idx / ppr, c = (idx % ppr) * PACK;
  const float* src = v + (long)(r / group_rows) * C + c;
  T* dst = out + (long)r * ldo + c;
  Vec16<T> o;
  if (accumulate) o.v = *(const decltype(o.v)*)dst;
#pragma unroll
  for (int e = 0; e < PACK; ++e) o.set(e, (accumulate ? o.get(e) : 0.f) + src[e] * scale);
  *(decltype(o.v)*)dst = o.v;
}

// ----------------------------------------------------------------------------------------- bilinear (align_corners=False)
DEVI void bil_src(int dst, float scale, int n_in, int& i0, int& i1, float& w1) {
  float s = ((float)dst + 0.5f) * scale - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  w1 = s - (float)i0;
}

// NHWC tokens [F][h][w][C] -> [F][H][W][C]  (F.interpolate / F.upsample bilinear of base18.py:102-103)
template <typename T>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const T* in, long ldi, T* out, long ldo, int F, int h, int w,
                                                            int H, int W, int C) {
  constexpr int PACK = TT<T>::PACK;
  const int ppr = C / PACK;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)F * H * W * ppr) return;
  const int c = (idx % ppr) * PACK;
  const long px = idx / ppr;
  const int x = px % W, y = (px / W) % H, f = px / ((long)W * H);
  int y0, y1, x0, x1; float wy, wx;
  bil_src(y, (float)h / H, h, y0, y1, wy);
  bil_src(x, (float)w / W, w, x0, x1, wx);
  const T* b = in + ((long)f * h * w) * ldi + c;
  Vec16<T> p00, p01, p10, p11, o;
  p00.v = *(const decltype(o.v)*)(b + ((long)y0 * w + x0) * ldi);
  p01.v = *(const decltype(o.v)*)(b + ((long)y0 * w + x1) * ldi);
  p10.v = *(const decltype(o.v)*)(b + ((long)y1 * w + x0) * ldi);
  p11.v = *(const decltype(o.v)*)(b + ((long)y1 * w + x1) * ldi);
#pragma unroll
  for (int e = 0; e < PACK; ++e)
    o.set(e, (1.f - wy) * ((1.f - wx) * p00.get(e) + wx * p01.get(e)) + wy * ((1.f - wx) * p10.get(e) + wx * p11.get(e)));
  *(decltype(o.v)*)(out + px * ldo + c) = o.v;
}

// gather-form backward: din[f][yi][xi][c] = sum over the output pixels that read (yi, xi)
template <typename T>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const T* dout, long ldo, T* din, long ldi, int F, int h, int w,
                                                            int H, int W, int C) {
  constexpr int PACK = TT<T>::PACK;
  const int ppr = C / PACK;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)F * h * w * ppr) return;
  const int c = (idx % ppr) * PACK;
  const long px = idx / ppr;
  const int xi = px % w, yi = (px / w) % h, f = px / ((long)w * h);
  const float sy = (float)h / H, sx = (float)w / W;
  const int ylo = max(0, (int)floorf(((float)yi - 0.5f) / sy - 0.5f) - 1), yhi = min(H - 1, (int)ceilf(((float)yi + 1.5f) / sy - 0.5f) + 1);
  const int xlo = max(0, (int)floorf(((float)xi - 0.5f) / sx - 0.5f) - 1), xhi = min(W - 1, (int)ceilf(((float)xi + 1.5f) / sx - 0.5f) + 1);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int y = ylo; y <= yhi; ++y) {
    int y0, y1; float wy;
    bil_src(y, sy, h, y0, y1, wy);
    const float cy = (y0 == yi ? 1.f - wy : 0.f) + (y1 == yi ? wy : 0.f);
    if (cy == 0.f) continue;
    for (int x = xlo; x <= xhi; ++x) {
      int x0, x1; float wx;
      bil_src(x, sx, w, x0, x1, wx);
      const float cx = (x0 == xi ? 1.f - wx : 0.f) + (x1 == xi ? wx : 0.f);
      if (cx == 0.f) continue;
      Vec16<T> d;
      d.v = *(const decltype(d.v)*)(dout + (((long)f * H + y) * W + x) * ldo + c);
#pragma unroll
      for (int e = 0; e < PACK; ++e) acc[e] += cy * cx * d.get(e);
    }
  }
  Vec16<T> o;
#pragma unroll
  for (int e = 0; e < PACK; ++e) o.set(e, acc[e]);
  *(decltype(o.v)*)(din + px * ldi + c) = o.v;
}

// tokens [F][h][w][nc] (pitch ldi) -> NCHW logits [F][nc][H][W]  (nn.functional.interpolate of base18.py:106)
template <typename T, typename TO>
__global__ __launch_bounds__(256) void logits_up_fwd_kernel(const T* in, long ldi, TO* out, int F, int h, int w, int H, int W,
                                                             int nc) {
  const long px = (long)blockIdx.x * 256 + threadIdx.x;
  if (px >= (long)F * H * W) return;
  const int x = px % W, y = (px / W) % H, f = px / ((long)W * H);
  int y0, y1, x0, x1; float wy, wx;
  bil_src(y, (float)h / H, h, y0, y1, wy);
  bil_src(x, (float)w / W, w, x0, x1, wx);
  const T* b = in + ((long)f * h * w) * ldi;
  const T* p00 = b + ((long)y0 * w + x0) * ldi; const T* p01 = b + ((long)y0 * w + x1) * ldi;
  const T* p10 = b + ((long)y1 * w + x0) * ldi; const T* p11 = b + ((long)y1 * w + x1) * ldi;
  for (int c = 0; c < nc; ++c) {
    const float v = (1.f - wy) * ((1.f - wx) * to_f32<T>(p00[c]) + wx * to_f32<T>(p01[c])) +
                    wy * ((1.f - wx) * to_f32<T>(p10[c]) + wx * to_f32<T>(p11[c]));
    out[(((long)f * nc + c) * H + y) * W + x] = from_f32<TO>(v);
  }
}

// backward, separable gather: dtok[f][yi][xi][c] = sum_y cy(yi,y) sum_x cx(xi,x) dlogits[f][c][y][x]
// one thread per (f, yi, xi, c); nc is small so the tensor is tiny and L2-resident.
template <typename T, typename TO>
__global__ __launch_bounds__(256) void logits_up_bwd_kernel(const TO* dout, T* din, long ldi, int F, int h, int w, int H, int W,
                                                             int nc) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long npx = (long)F * h * w;
  if (idx >= npx * nc) return;
  // neighbouring lanes = neighbouring low-resolution pixels of ONE class plane: their gather windows are adjacent stretches of
  // the same high-resolution rows (with the class as the fastest index every lane read a different plane: 82 us for 25 MB)
  const int c = (int)(idx / npx);
  const long px = idx - (long)c * npx;
  const int xi = px % w, yi = (px / w) % h, f = px / ((long)w * h);
  const float sy = (float)h / H, sx = (float)w / W;
  const int ylo = max(0, (int)floorf(((float)yi - 0.5f) / sy - 0.5f) - 1), yhi = min(H - 1, (int)ceilf(((float)yi + 1.5f) / sy - 0.5f) + 1);
  const int xlo = max(0, (int)floorf(((float)xi - 0.5f) / sx - 0.5f) - 1), xhi = min(W - 1, (int)ceilf(((float)xi + 1.5f) / sx - 0.5f) + 1);
  const TO* plane = dout + ((long)f * nc + c) * H * W;
  float acc = 0.f;
  for (int y = ylo; y <= yhi; ++y) {
    int y0, y1; float wy;
    bil_src(y, sy, h, y0, y1, wy);
    const float cy = (y0 == yi ? 1.f - wy : 0.f) + (y1 == yi ? wy : 0.f);
    if (cy == 0.f) continue;
    float row = 0.f;
    for (int x = xlo; x <= xhi; ++x) {
      int x0, x1; float wx;
      bil_src(x, sx, w, x0, x1, wx);
      const float cx = (x0 == xi ? 1.f - wx : 0.f) + (x1 == xi ? wx : 0.f);
      if (cx != 0.f) row += cx * to_f32<TO>(plane[(long)y * W + x]);
    }
    acc += cy * row;
  }
  din[px * ldi + c] = from_f32<T>(acc);
}

// ----------------------------------------------------------------------------------------- OHEM cross entropy
// per-pixel CE (ignore_index -> 0) + the scalars the OHEM rule needs: stats[0] = #(loss > thresh), stats[2..3] = sum of those
// losses (fixed point, below).   losses.py:32-34.  A label outside [0, nc) that is not ignore_index (the reference raises) is never
// used as an index: its loss is NaN (so it is neither counted nor selected, and ce_bwd gives it no gradient) and stats[1] counts it,
// which makes ohem_final_kernel return NaN - the error reaches the caller without a host sync.
DEVI unsigned long long loss_to_fix(float v) { return (unsigned long long)((double)fmaxf(v, 0.f) * 4294967296.0); }
DEVI float fix_to_loss(unsigned long long f) { return (float)((double)f * (1.0 / 4294967296.0)); }

template <typename TL>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const TL* logits, const long* labels, float* loss, float* stats, int F,
                                                      long HW, int nc, int ignore_index, float thresh) {
  // grid-stride over the pixels: at one pixel per thread the 4096 workgroups of a 4 x 512 x 512 batch ended in 8192 same-address
  // fp32 atomics (~40 ns each, serialised at the memory side): 114 us for a 62 MB pass
  float hc = 0.f, hs = 0.f, nbad = 0.f;
  const long n = (long)F * HW;
  for (long px = (long)blockIdx.x * 256 + threadIdx.x; px < n; px += (long)gridDim.x * 256) {
    float l = 0.f;
    const long f = px / HW, p = px % HW;
    const long lab = labels[px];
    if (lab != ignore_index && (lab < 0 || lab >= nc)) {
      l = __builtin_nanf("");
      nbad += 1.f;
    } else if (lab != ignore_index) {
      const TL* b = logits + f * nc * HW + p;
      float mx = -3.0e38f;
      int am = 0;
      for (int c = 0; c < nc; ++c) {
        const float v = to_f32<TL>(b[(long)c * HW]);
        if (v > mx) { mx = v; am = c; }
      }
      float s = 0.f;                                   // sum over the classes other than the arg-max: log-sum-exp = mx + log1p(s)
      for (int c = 0; c < nc; ++c)
        if (c != am) s += expf(to_f32<TL>(b[(long)c * HW]) - mx);
      // loss = (mx - x[lab]) + log1p(s).  The old mx + log(1 + s) - x[lab] lost ~ulp(|mx|) / 2 when the label is the arg-max (the
      // small log(1 + s) added to |mx| and taken back out: 1e-6 at |logit| 20 on a loss of 1e-4), and log(1 + s) itself lost s
      // below ulp(1) / 2: both vanish here (mx - x[lab] is exact or 0; log1p keeps the relative accuracy of s)
      l = (mx - to_f32<TL>(b[lab * HW])) + log1pf(s);
    }
    loss[px] = l;
    if (l > thresh) { hc += 1.f; hs += l; }
  }
  float cnt = wave_sum(hc), sm = wave_sum(hs), bad = wave_sum(nbad);
  __shared__ float red[3][4];
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = cnt; red[1][threadIdx.x >> 6] = sm; red[2][threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float nb = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    if (nb != 0.f) atomicAdd(stats + 1, nb);
    // stats[0]: a count (integers < 2^24: exact in fp32, so the atomic sum does not depend on the order); the SUM goes to the 64-bit
    // fixed-point accumulator at stats[2..3] (2^-32 units; losses are >= 0 and n * max loss < 2^32): integer adds are associative,
    // so two runs give the same bits whatever the order the workgroups finish in
    atomicAdd(stats + 0, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    atomicAdd((unsigned long long*)(stats + 2), loss_to_fix(red[1][0] + red[1][1] + red[1][2] + red[1][3]));
  }
}

// dlogits = g * w(px) * (softmax - onehot),  w = sel[1] if loss(px) > sel[0], sel[3] if loss(px) == sel[0], else 0   (sel on device:
// no host sync; see ohem_final_kernel).  A NaN loss (a label outside [0, nc)) compares false both ways: no gradient.
template <typename TL>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const TL* logits, const long* labels, const float* loss, const float* sel,
                                                      const float* gscale, TL* dlogits, int F, long HW, int nc,
                                                      int ignore_index) {
  const long px = (long)blockIdx.x * 256 + threadIdx.x;
  if (px >= (long)F * HW) return;
  const long f = px / HW, p = px % HW;
  const long lab = labels[px];
  const float l = loss[px];
  const float w = l > sel[0] ? sel[1] : (l == sel[0] ? sel[3] : 0.f);
  const float wgt = (w != 0.f && lab != ignore_index && lab >= 0 && lab < nc) ? w * gscale[0] : 0.f;
  const TL* b = logits + f * nc * HW + p;
  TL* d = dlogits + f * nc * HW + p;
  if (wgt == 0.f) {
    for (int c = 0; c < nc; ++c) d[(long)c * HW] = from_f32<TL>(0.f);
    return;
  }
  float mx = -3.0e38f;
  for (int c = 0; c < nc; ++c) mx = fmaxf(mx, to_f32<TL>(b[(long)c * HW]));
  float s = 0.f;
  for (int c = 0; c < nc; ++c) s += expf(to_f32<TL>(b[(long)c * HW]) - mx);
  const float inv = 1.f / s;
  for (int c = 0; c < nc; ++c) {
    const float pr = expf(to_f32<TL>(b[(long)c * HW]) - mx) * inv;
    d[(long)c * HW] = from_f32<TL>(wgt * (pr - (c == lab ? 1.f : 0.f)));
  }
}

// ------------------------------------------------------------------------------------------------ C ABI
#define PACK_OF(dt) ((dt) == 0 ? 8 : 4)
#define DISPATCH_T(dt, CALL_BF16, CALL_F32) do { if ((dt) == 0) { CALL_BF16; } else { CALL_F32; } } while (0)

static int colstats_geometry(int dtype, int M, int C, int groups, int unit_rows, int* cpb_o, int* rpc_o, int* cpg_o) {
  if (C % PACK_OF(dtype) || groups <= 0 || M % groups) return -1401;
  if (unit_rows > 0 && M % ((long)groups * unit_rows)) return -1405;
  const int ppr = C / PACK_OF(dtype), cpb = pick_cpb(ppr);
  const int gr = M / groups, rpc = fit_chunk(reduce_rows_per_chunk(gr, groups * ((ppr + cpb - 1) / cpb), 256 / cpb), unit_rows);
  if (rpc <= 0) return -1405;
  *cpb_o = cpb; *rpc_o = rpc; *cpg_o = (gr + rpc - 1) / rpc;
  return 0;
}
/* floats of scratch stswin_colstats needs for this geometry ([groups * chunks][2][C]); < 0: invalid geometry */
extern "C" long stswin_colstats_scratch(int dtype, int M, int C, int groups, int unit_rows) {
  int cpb, rpc, cpg;
  const int rc = colstats_geometry(dtype, M, C, groups, unit_rows, &cpb, &rpc, &cpg);
  return rc ? rc : (long)groups * cpg * 2 * C;
}

extern "C" int stswin_colstats(int dtype, const void* x, long ldx, float* sum, float* sumsq, int M, int C, int groups,
                               int unit_rows, float* scratch, void* stream) {
  int cpb, rpc, cpg;
  const int rc = colstats_geometry(dtype, M, C, groups, unit_rows, &cpb, &rpc, &cpg);
  if (rc) return rc;
  if (ldx % PACK_OF(dtype)) return -1401;
  if (!scratch) return -1406;
  const int ppr = C / PACK_OF(dtype), gr = M / groups;
  dim3 grid((ppr + cpb - 1) / cpb, groups * cpg);
  hipStream_t st = (hipStream_t)stream;
  if (sumsq)
    DISPATCH_T(dtype, hipLaunchKernelGGL((colstats_kernel<bf16, true>), grid, dim3(256), 0, st, (const bf16*)x, ldx, scratch, C, gr, cpg, rpc, cpb, unit_rows),
               hipLaunchKernelGGL((colstats_kernel<float, true>), grid, dim3(256), 0, st, (const float*)x, ldx, scratch, C, gr, cpg, rpc, cpb, unit_rows));
  else
    DISPATCH_T(dtype, hipLaunchKernelGGL((colstats_kernel<bf16, false>), grid, dim3(256), 0, st, (const bf16*)x, ldx, scratch, C, gr, cpg, rpc, cpb, unit_rows),
               hipLaunchKernelGGL((colstats_kernel<float, false>), grid, dim3(256), 0, st, (const float*)x, ldx, scratch, C, gr, cpg, rpc, cpb, unit_rows));
  // sum[g] | sumsq[g] += the group's chunk slabs, in chunk order
  const int rf = stswin_fold_launch(scratch, 2L * C, (long)cpg * 2 * C, cpg, C, sumsq ? 2 : 1, sum, sumsq, nullptr, C, groups, 1, st);
  if (rf) return rf;
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_bn_finalize(int dtype, const void* x, long ldx, const float* sum, const float* sumsq, float* mean,
                                  float* rstd, float* running_mean, float* running_var, int M, int C, int groups, float eps,
                                  float momentum, int unit_rows, void* stream) {
  if (groups <= 0 || M % groups) return -1401;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((C + 255) / 256);
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_finalize_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, ldx, sum, sumsq, mean, rstd, running_mean, running_var, C, groups, M / groups, eps, momentum, unit_rows),
             hipLaunchKernelGGL(bn_finalize_kernel<float>, grid, dim3(256), 0, st, (const float*)x, ldx, sum, sumsq, mean, rstd, running_mean, running_var, C, groups, M / groups, eps, momentum, unit_rows));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_bn_apply(int dtype, const void* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, const void* resid, long ldr, void* y, long ldy, int M, int C, int groups,
                               int relu, int unit_rows, void* stream) {
  const int pk = PACK_OF(dtype);
  if (C % pk || ldx % pk || ldy % pk || (resid && ldr % pk) || groups <= 0 || M % groups) return -1402;
  const int ppr = C / pk, cpb = pick_cpb(ppr);
  if (unit_rows > 0 && M % ((long)groups * unit_rows)) return -1405;
  const int gr = M / groups, rpc = fit_chunk(8 * (256 / cpb), unit_rows);
  if (rpc <= 0) return -1405;
  const int cpg = (gr + rpc - 1) / rpc;
  dim3 grid((ppr + cpb - 1) / cpb, groups * cpg);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_apply_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, ldx, mean, rstd, gamma, beta, (const bf16*)resid, ldr, (bf16*)y, ldy, C, gr, cpg, rpc, relu, cpb, unit_rows),
             hipLaunchKernelGGL(bn_apply_kernel<float>, grid, dim3(256), 0, st, (const float*)x, ldx, mean, rstd, gamma, beta, (const float*)resid, ldr, (float*)y, ldy, C, gr, cpg, rpc, relu, cpb, unit_rows));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

static int bn_bwd_geometry(int dtype, int M, int C, int groups, int unit_rows, int* cpb_o, int* rpc_o, int* rpc2_o) {
  const int pk = PACK_OF(dtype);
  if (C % pk || groups <= 0 || M % groups) return -1403;
  if (unit_rows > 0 && M % ((long)groups * unit_rows)) return -1405;
  const int ppr = C / pk, cpb = pick_cpb(ppr), xb = (ppr + cpb - 1) / cpb, nrl = 256 / cpb;
  const int rpc = fit_chunk(bn_bwd_rows(M, xb, nrl, 64) * nrl, unit_rows);
  const int rpc2 = fit_chunk(bn_bwd_rows(M, xb, nrl, 32) * nrl, unit_rows);
  if (rpc <= 0 || rpc2 <= 0) return -1405;
  *cpb_o = cpb; *rpc_o = rpc; *rpc2_o = rpc2;
  return 0;
}
/* floats of scratch the reduce pass of stswin_bn_bwd needs ([groups * chunks][2][C]); < 0: invalid geometry */
extern "C" long stswin_bn_bwd_scratch(int dtype, int M, int C, int groups, int unit_rows) {
  int cpb, rpc, rpc2;
  const int rc = bn_bwd_geometry(dtype, M, C, groups, unit_rows, &cpb, &rpc, &rpc2);
  return rc ? rc : (long)groups * ((M / groups + rpc - 1) / rpc) * 2 * C;
}

extern "C" int stswin_bn_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, const void* y, long ldy,
                             const float* mean, const float* rstd, const float* gamma, const float* beta, float* s1, float* s2,
                             void* dx, long lddx, void* dresid, long lddr, int M, int C, int groups, int relu, int training,
                             int phase, long rows_total, int unit_rows, float* gsum, float* scratch, void* stream) {
  const int pk = PACK_OF(dtype);
  int cpb, rpc, rpc2;
  const int rc = bn_bwd_geometry(dtype, M, C, groups, unit_rows, &cpb, &rpc, &rpc2);
  if (rc) return rc;
  if (ldx % pk || lddy % pk || lddx % pk || (relu && y && ldy % pk)) return -1403;
  if (relu && !y && !beta) return -1404;               // no stored output: the mask is recomputed and needs beta
  if (phase != 2 && !scratch) return -1406;
  const int ppr = C / pk, gr = M / groups;
  const int cpg = (gr + rpc - 1) / rpc;
  dim3 g1((ppr + cpb - 1) / cpb, groups * cpg);
  const int cpg2 = (gr + rpc2 - 1) / rpc2;
  dim3 g2((ppr + cpb - 1) / cpb, groups * cpg2);
  hipStream_t st = (hipStream_t)stream;
  const float inv_n = 1.0f / (float)(rows_total > 0 ? rows_total : gr);
  if (phase != 2) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(bn_bwd_reduce_kernel<bf16>, g1, dim3(256), 0, st, (const bf16*)dy, lddy, (const bf16*)x, ldx, (const bf16*)y, ldy, mean, rstd, scratch, C, gr, cpg, rpc, relu, cpb, gamma, beta, unit_rows),
               hipLaunchKernelGGL(bn_bwd_reduce_kernel<float>, g1, dim3(256), 0, st, (const float*)dy, lddy, (const float*)x, ldx, (const float*)y, ldy, mean, rstd, scratch, C, gr, cpg, rpc, relu, cpb, gamma, beta, unit_rows));
    // s1[g] | s2[g] += the group's chunk slabs, in chunk order (deterministic; s1 / s2 arrive zeroed)
    const int rf = stswin_fold_launch(scratch, 2L * C, (long)cpg * 2 * C, cpg, C, 2, s1, s2, nullptr, C, groups, 1, st);
    if (rf) return rf;
  }
  if (phase != 1)
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_bwd_dx_kernel<bf16>, g2, dim3(256), 0, st, (const bf16*)dy, lddy, (const bf16*)x, ldx, (const bf16*)y, ldy, mean, rstd, gamma, s1, s2, (bf16*)dx, lddx, (bf16*)dresid, lddr, C, gr, cpg2, rpc2, relu, training, cpb, inv_n, beta, unit_rows, gsum),
             hipLaunchKernelGGL(bn_bwd_dx_kernel<float>, g2, dim3(256), 0, st, (const float*)dy, lddy, (const float*)x, ldx, (const float*)y, ldy, mean, rstd, gamma, s1, s2, (float*)dx, lddx, (float*)dresid, lddr, C, gr, cpg2, rpc2, relu, training, cpb, inv_n, beta, unit_rows, gsum));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// BatchNorm (batch or running statistics of `groups` statistic groups) + ReLU + nn.MaxPool2d(3, 2, 1) in one pass over the
// BatchNorm's input: out [frames*Hp*Wp][C], arg = winning tap per value (first maximum in (ky, kx) scan order, like torch and
// like maxpool_fwd_kernel).  Each candidate is bn_apply_kernel's expression rounded to T before it is compared, so output and
// taps are those of the two-pass form.  torchvision resnet18 conv1 -> bn1 -> relu -> maxpool, resnet.py:98-102.
template <typename T>
__global__ __launch_bounds__(256) void bn_relu_pool_kernel(const T* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                                                            const float* beta, T* out, long ldo, unsigned char* arg, int frames, int H,
                                                            int W, int Hp, int Wp, int C, int G, int group_rows, int unit) {
  // A thread owns a 2 x 2 block of pooled pixels of one 16-byte channel chunk: their windows share a 5 x 5 patch of the input
  // (25 loads and BatchNorm evaluations instead of 36), scanned row by row so every output meets its taps in (ky, kx) order.
  constexpr int PACK = TT<T>::PACK;
  const int ppr = C / PACK, Hb = (Hp + 1) >> 1, Wb = (Wp + 1) >> 1;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)frames * Hb * Wb * ppr) return;
  const int c = (int)(idx % ppr) * PACK;
  const long pb = idx / ppr;
  const int xb = (int)(pb % Wb), yb = (int)((pb / Wb) % Hb);
  const long f = pb / ((long)Wb * Hb);
  const long row0 = f * H * W;
  const int g = unit > 0 ? (int)((row0 / unit) % G) : (int)(row0 / group_rows);
  float sc[8], sh[8], best[4][8];
  unsigned char ba[4][8];
#pragma unroll
  for (int e = 0; e < PACK; ++e) {
    const float rs = rstd[(long)g * C + c + e] * gamma[c + e];
    sc[e] = rs;
    sh[e] = beta[c + e] - mean[(long)g * C + c + e] * rs;
#pragma unroll
    for (int o = 0; o < 4; ++o) { best[o][e] = -3.0e38f; ba[o][e] = 255; }
  }
  const int y0 = 4 * yb - 1, x0 = 4 * xb - 1;           // input coordinates of the patch origin (pooled (2 yb, 2 xb), tap (0, 0))
#pragma unroll
  for (int iy = 0; iy < 5; ++iy) {
    const int yy = y0 + iy;
    if (yy < 0 || yy >= H) continue;
#pragma unroll
    for (int ix = 0; ix < 5; ++ix) {
      const int xx = x0 + ix;
      if (xx < 0 || xx >= W) continue;
      Vec16<T> v, z;
      v.v = *(const decltype(v.v)*)(x + (row0 + (long)yy * W + xx) * ldx + c);
#pragma unroll
      for (int e = 0; e < PACK; ++e) z.set(e, fmaxf(v.get(e) * sc[e] + sh[e], 0.f));
#pragma unroll
      for (int oy = 0; oy < 2; ++oy) {
        const int ky = iy - 2 * oy;                      // tap row of this input row in output row 2 yb + oy
        if (ky < 0 || ky > 2) continue;
#pragma unroll
        for (int ox = 0; ox < 2; ++ox) {
          const int kx = ix - 2 * ox;
          if (kx < 0 || kx > 2) continue;
          const int o = oy * 2 + ox;
          const unsigned char t = (unsigned char)(ky * 3 + kx);
#pragma unroll
          for (int e = 0; e < PACK; ++e) {
            const float u = z.get(e);
            if (u > best[o][e] || ba[o][e] == 255) { best[o][e] = u; ba[o][e] = t; }
          }
        }
      }
    }
  }
#pragma unroll
  for (int oy = 0; oy < 2; ++oy)
#pragma unroll
    for (int ox = 0; ox < 2; ++ox) {
      const int yo = 2 * yb + oy, xo = 2 * xb + ox, o = oy * 2 + ox;
      if (yo >= Hp || xo >= Wp) continue;
      const long px = (f * Hp + yo) * Wp + xo;
      Vec16<T> r;
      unsigned a[2] = {0, 0};
#pragma unroll
      for (int e = 0; e < PACK; ++e) { r.set(e, best[o][e]); a[e >> 2] |= (unsigned)ba[o][e] << (8 * (e & 3)); }
      if (PACK == 8) *(uint2*)(arg + px * C + c) = uint2{a[0], a[1]};
      else *(unsigned*)(arg + px * C + c) = a[0];
      *(decltype(r.v)*)(out + px * ldo + c) = r.v;
    }
}

extern "C" int stswin_bn_relu_pool(int dtype, const void* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, void* out, long ldo, unsigned char* arg, int frames, int H, int W, int C, int groups,
                                   int unit_rows, void* stream) {
  const int pk = PACK_OF(dtype);
  const long M = (long)frames * H * W;
  if (frames <= 0 || H <= 0 || W <= 0 || C % pk || ldx % pk || ldo % pk || groups <= 0 || M % groups) return -1408;
  if (unit_rows > 0 ? (unit_rows % ((long)H * W) != 0 || M % ((long)groups * unit_rows)) : ((M / groups) % ((long)H * W) != 0)) return -1408;
  const int Hp = (H - 1) / 2 + 1, Wp = (W - 1) / 2 + 1;
  const long n = (long)frames * ((Hp + 1) / 2) * ((Wp + 1) / 2) * (C / pk);
  dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_relu_pool_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, ldx, mean, rstd, gamma, beta, (bf16*)out, ldo, arg, frames, H, W, Hp, Wp, C, groups, (int)(M / groups), unit_rows),
             hipLaunchKernelGGL(bn_relu_pool_kernel<float>, grid, dim3(256), 0, st, (const float*)x, ldx, mean, rstd, gamma, beta, (float*)out, ldo, arg, frames, H, W, Hp, Wp, C, groups, (int)(M / groups), unit_rows));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_rows_broadcast(int dtype, const float* v, void* out, long ldo, int M, int C, int groups, float scale,
                                     int accumulate, void* stream) {
  const int pk = PACK_OF(dtype);
  if (C % pk || ldo % pk || groups <= 0 || M % groups) return -1404;
  const long n = (long)M * (C / pk);
  dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(rows_broadcast_kernel<bf16>, grid, dim3(256), 0, st, v, (bf16*)out, ldo, M, C, M / groups, scale, accumulate),
             hipLaunchKernelGGL(rows_broadcast_kernel<float>, grid, dim3(256), 0, st, v, (float*)out, ldo, M, C, M / groups, scale, accumulate));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_bilinear(int dtype, const void* in, long ldi, void* out, long ldo, int frames, int h, int w, int H, int W,
                               int C, int backward, void* stream) {
  /* forward: in [F][h][w][C] -> out [F][H][W][C];  backward: `in` = d(out) [F][H][W][C] (pitch ldi), `out` = d(in) (pitch ldo) */
  const int pk = PACK_OF(dtype);
  if (C % pk || ldi % pk || ldo % pk) return -1405;
  hipStream_t st = (hipStream_t)stream;
  if (!backward) {
    const long n = (long)frames * H * W * (C / pk);
    dim3 grid((unsigned)((n + 255) / 256));
    DISPATCH_T(dtype, hipLaunchKernelGGL(bilinear_fwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)in, ldi, (bf16*)out, ldo, frames, h, w, H, W, C),
               hipLaunchKernelGGL(bilinear_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)in, ldi, (float*)out, ldo, frames, h, w, H, W, C));
  } else {
    const long n = (long)frames * h * w * (C / pk);
    dim3 grid((unsigned)((n + 255) / 256));
    DISPATCH_T(dtype, hipLaunchKernelGGL(bilinear_bwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)in, ldi, (bf16*)out, ldo, frames, h, w, H, W, C),
               hipLaunchKernelGGL(bilinear_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)in, ldi, (float*)out, ldo, frames, h, w, H, W, C));
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_logits_upsample(int dtype, const void* tokens, long ldt, void* nchw, int frames, int h, int w, int H,
                                      int W, int nc, int backward, void* stream) {
  /* forward: tokens [F][h][w][nc] -> nchw [F][nc][H][W] (same dtype); backward: nchw = dlogits -> tokens = d(tokens) */
  hipStream_t st = (hipStream_t)stream;
  if (!backward) {
    const long n = (long)frames * H * W;
    dim3 grid((unsigned)((n + 255) / 256));
    DISPATCH_T(dtype, hipLaunchKernelGGL((logits_up_fwd_kernel<bf16, bf16>), grid, dim3(256), 0, st, (const bf16*)tokens, ldt, (bf16*)nchw, frames, h, w, H, W, nc),
               hipLaunchKernelGGL((logits_up_fwd_kernel<float, float>), grid, dim3(256), 0, st, (const float*)tokens, ldt, (float*)nchw, frames, h, w, H, W, nc));
  } else {
    const long n = (long)frames * h * w * nc;
    dim3 grid((unsigned)((n + 255) / 256));
    DISPATCH_T(dtype, hipLaunchKernelGGL((logits_up_bwd_kernel<bf16, bf16>), grid, dim3(256), 0, st, (const bf16*)nchw, (bf16*)tokens, ldt, frames, h, w, H, W, nc),
               hipLaunchKernelGGL((logits_up_bwd_kernel<float, float>), grid, dim3(256), 0, st, (const float*)nchw, (float*)tokens, ldt, frames, h, w, H, W, nc));
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_ce_fwd(int dtype, const void* logits, const long* labels, float* loss, float* stats, int frames, long HW,
                             int nc, int ignore_index, float thresh, void* stream) {
  const long n = (long)frames * HW;
  const long want = (n + 255) / 256;
  dim3 grid((unsigned)(want < 1024 ? want : 1024));        // grid-stride: <= 2048 atomics on the two counters per call
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(ce_fwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)logits, labels, loss, stats, frames, HW, nc, ignore_index, thresh),
             hipLaunchKernelGGL(ce_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, labels, loss, stats, frames, HW, nc, ignore_index, thresh));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_ce_bwd(int dtype, const void* logits, const long* labels, const float* loss, const float* sel,
                             const float* gscale, void* dlogits, int frames, long HW, int nc, int ignore_index, void* stream) {
  const long n = (long)frames * HW;
  dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(ce_bwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)logits, labels, loss, sel, gscale, (bf16*)dlogits, frames, HW, nc, ignore_index),
             hipLaunchKernelGGL(ce_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, labels, loss, sel, gscale, (float*)dlogits, frames, HW, nc, ignore_index));
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// ----------------------------------------------------------------------------------------- a15: OHEM selection
// OhemCELoss2D (seg18/utils/losses.py:32-40) sorts all B*H*W pixel losses to read loss[n_min] and, when that is not above
// the threshold, to average the n_min largest.  Here: #(loss > thresh) comes from ce_fwd (the branch test), and the mean
// of the n_min largest from an exact 3-level radix select over the float bits (losses are >= 0, so the bit patterns
// order like the values): per level a 2048-bin (11 + 11 + 10 bits) histogram of counts AND sums, restricted to the
// prefix found by the previous level, gives the k-th largest value and the sum of everything above it:
//   mean = (sum_above + k_rem * kth) / n_min.
// Three passes over the 4 MB loss vector (L2 resident) + one block of bookkeeping instead of a 1 M-element top-k; every
// pass returns at once when the threshold branch is taken (stats[0] > n_min).
// sel (for ce_bwd) = (cut, weight above the cut, 1 if the top-n_min branch was taken, weight AT the cut).  Threshold branch: cut =
// thresh, weight 1 / n_hard above it, 0 at it.  Top-n_min branch: cut = kth, 1 / n_min above it; the t losses equal to kth share the
// k_rem places left, k_rem / (t * n_min) each - the reference's sort-then-slice gradient averaged over the orders of the tied pixels
// (its value, sum_above + k_rem * kth, does not depend on that order).  Level 2 resolves all 31 key bits, so its bin count is t.
struct OhemWork {                       // zeroed by the launcher
  unsigned cnt[3][2048];
  unsigned long long sum[3][2048];      // sums of the losses per bin in 2^-32 fixed point (see loss_to_fix): integer atomics are
                                        // associative, so the selected mean does not depend on the order the workgroups finish in
  unsigned long long sabove[3];         // per level: sum (fixed point) of everything above the level's prefix bin
  unsigned state[3][2];                 // per level: prefix, k (still to take at this level)
};

// k-th largest over `nbins` bins (from the top): bin with count(above) < k <= count(above) + count(bin); 256 threads
__device__ void ohem_scan(const unsigned* cnt, const unsigned long long* sum, int nbins, unsigned k, unsigned* out /* LDS [2]: bin, k_rem */,
                          unsigned long long* out_sum /* LDS [1]: sum above the bin */) {
  __shared__ unsigned pc[256];
  __shared__ unsigned long long ps[256];
  const int t = threadIdx.x, per = nbins / 256;
  unsigned c = 0;
  unsigned long long sm = 0;
  for (int b = 0; b < per; ++b) { c += cnt[nbins - 1 - (t * per + b)]; sm += sum[nbins - 1 - (t * per + b)]; }
  pc[t] = c; ps[t] = sm;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                 // inclusive scan over threads (thread 0 = highest bins)
    const unsigned c2 = t >= d ? pc[t - d] : 0u;
    const unsigned long long s2 = t >= d ? ps[t - d] : 0ull;
    __syncthreads();
    pc[t] += c2; ps[t] += s2;
    __syncthreads();
  }
  const unsigned incl = pc[t], excl = incl - c;
  if (excl < k && k <= incl) {                         // exactly one thread
    unsigned above = excl;
    unsigned long long sabove = ps[t] - sm;
    for (int b = 0; b < per; ++b) {
      const int bin = nbins - 1 - (t * per + b);
      const unsigned cb = cnt[bin];
      if (above + cb >= k) { out[0] = (unsigned)bin; out[1] = k - above; out_sum[0] = sabove; break; }
      above += cb; sabove += sum[bin];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* loss, long n, long n_min, const float* stats, OhemWork* wk, int level) {
  if (stats[0] > (float)n_min) return;                 // threshold branch: the top-k mean is not needed
  __shared__ unsigned hc[2048];
  __shared__ unsigned long long hs[2048];
  __shared__ unsigned sc[2];
  __shared__ unsigned long long ssum[1];
  for (int i = threadIdx.x; i < 2048; i += 256) { hc[i] = 0u; hs[i] = 0ull; }
  unsigned prefix = 0;
  if (level > 0) {
    const unsigned k = level == 1 ? (unsigned)n_min : wk->state[1][1];
    ohem_scan(wk->cnt[level - 1], wk->sum[level - 1], 2048, k, sc, ssum);
    const unsigned up = level == 1 ? 0u : wk->state[1][0];
    prefix = level == 1 ? sc[0] : ((up << 11) | sc[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const unsigned long long sprev = level == 1 ? 0ull : wk->sabove[1];
      wk->state[level][0] = prefix; wk->state[level][1] = sc[1]; wk->sabove[level] = sprev + ssum[0];
    }
  }
  __syncthreads();
  const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
  const unsigned mask = level == 2 ? 1023u : 2047u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = loss[i];
    const unsigned key = __float_as_uint(v) & 0x7fffffffu;
    const bool in = level == 0 || (level == 1 ? (key >> 21) == prefix : (key >> 10) == prefix);
    if (in) { const unsigned b = (key >> shift) & mask; atomicAdd(&hc[b], 1u); atomicAdd(&hs[b], loss_to_fix(v)); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2048; i += 256)
    if (hc[i]) { atomicAdd(&wk->cnt[level][i], hc[i]); atomicAdd(&wk->sum[level][i], hs[i]); }
}

__global__ __launch_bounds__(256) void ohem_final_kernel(long n_min, float thresh, const float* stats, const OhemWork* wk, float* value,
                                                         float* sel) {
  const float n_hard = stats[0];
  const bool bad = stats[1] != 0.f;                    // labels outside [0, nc): no defined loss (ce_fwd_kernel)
  if (n_hard > (float)n_min) {                         // loss[n_min] > thresh: mean over loss > thresh
    if (threadIdx.x == 0) {
      const float inv = 1.f / fmaxf(n_hard, 1.f);
      value[0] = bad ? __builtin_nanf("") : fix_to_loss(*(const unsigned long long*)(stats + 2)) * inv;
      sel[0] = thresh; sel[1] = inv; sel[2] = 0.f; sel[3] = 0.f;
    }
    return;
  }
  __shared__ unsigned sc[2];
  __shared__ unsigned long long ssum[1];
  ohem_scan(wk->cnt[2], wk->sum[2], 1024, wk->state[2][1], sc, ssum);
  if (threadIdx.x == 0) {
    const float kth = __uint_as_float((wk->state[2][0] << 10) | sc[0]);
    const float total = fix_to_loss(wk->sabove[2] + ssum[0]) + (float)sc[1] * kth;
    const unsigned ties = wk->cnt[2][sc[0]];           // >= k_rem = sc[1] >= 1
    value[0] = bad ? __builtin_nanf("") : total / (float)n_min;
    sel[0] = kth; sel[1] = 1.f / (float)n_min; sel[2] = 1.f;
    sel[3] = (float)((double)sc[1] / ((double)ties * (double)n_min));
  }
}

extern "C" int stswin_ohem_select(const float* loss, long n, long n_min, float thresh, const float* stats, void* work,
                                  long work_bytes, float* value, float* sel, void* stream) {
  if (n <= 0 || n_min <= 0 || n_min > n) return -1301;
  if (work_bytes < (long)sizeof(OhemWork)) return -1302;
  hipStream_t st = (hipStream_t)stream;
  stswin_zero_bytes(work, sizeof(OhemWork), st);         // (a kernel, not hipMemsetAsync: see common.h)
  const unsigned grid = (unsigned)max(1L, min(512L, (n + 4095) / 4096));
  for (int level = 0; level < 3; ++level)
    hipLaunchKernelGGL(ohem_hist_kernel, dim3(grid), dim3(256), 0, st, loss, n, n_min, stats, (OhemWork*)work, level);
  hipLaunchKernelGGL(ohem_final_kernel, dim3(1), dim3(256), 0, st, n_min, thresh, stats, (const OhemWork*)work, value, sel);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// ----------------------------------------------------------------------------------------- f4: inference post-processing
// seg18/test.py:153-158: F.interpolate(out, (H, W), bilinear, align_corners=True) -> softmax -> argmax, then Dice / IoU
// (utils/EndoMetric.py).  One pass: interpolate the nc logits of an output pixel in registers, take the arg-max (softmax
// is monotone, so it is skipped), write the label, and - when ground truth is given - count per frame and class
// |gt == c|, |pred == c| and |gt == c and pred == c| (LDS histogram per block, one atomic per non-zero bin).
template <typename TL>
__global__ __launch_bounds__(256) void upsample_argmax_kernel(const TL* logits, unsigned char* labels, const long* gt,
                                                              int* counts, int F, int nc, int h, int w, int H, int W) {
  __shared__ int hist[3 * 64];
  for (int i = threadIdx.x; i < 3 * 64; i += 256) hist[i] = 0;
  __syncthreads();
  const long per_frame = (long)H * W;
  const long blocks_per_frame = (per_frame + 255) / 256;
  const int f = blockIdx.x / blocks_per_frame;
  const long px = (blockIdx.x % blocks_per_frame) * 256 + threadIdx.x;
  if (px < per_frame) {
    const int x = px % W, y = px / W;
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float fy = y * sy, fx = x * sx;
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float wy = fy - y0, wx = fx - x0;
    const TL* b = logits + (long)f * nc * h * w;
    float best = -3.0e38f; int arg = 0;
    for (int c = 0; c < nc; ++c) {
      const TL* pl = b + (long)c * h * w;
      const float v = (1.f - wy) * ((1.f - wx) * to_f32<TL>(pl[y0 * w + x0]) + wx * to_f32<TL>(pl[y0 * w + x1])) +
                      wy * ((1.f - wx) * to_f32<TL>(pl[y1 * w + x0]) + wx * to_f32<TL>(pl[y1 * w + x1]));
      if (v > best) { best = v; arg = c; }
    }
    labels[(long)f * per_frame + px] = (unsigned char)arg;
    if (gt) {
      const long g = gt[(long)f * per_frame + px];          // compared as int64: 2^32 + 3 is no class, as in the two kernels below
      if (g >= 0 && g < 64) atomicAdd(&hist[(int)g], 1);
      atomicAdd(&hist[64 + arg], 1);
      if (g == (long)arg) atomicAdd(&hist[128 + arg], 1);
    }
  }
  if (gt) {
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 64; i += 256) {
      const int k = i / 64, c = i % 64;
      if (c < nc && hist[i]) atomicAdd(counts + ((long)f * 3 + k) * nc + c, hist[i]);
    }
  }
}

extern "C" int stswin_upsample_argmax(int dtype, const void* logits, unsigned char* labels, const long* gt, int* counts,
                                      int frames, int nc, int h, int w, int H, int W, void* stream) {
  if (nc <= 0 || nc > 64 || frames <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return -1406;
  if (logits == nullptr || labels == nullptr || (gt != nullptr && counts == nullptr)) return -1406;
  const long bpf = ((long)H * W + 255) / 256;
  dim3 grid((unsigned)(bpf * frames));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) hipLaunchKernelGGL(upsample_argmax_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)logits, labels, gt, counts, frames, nc, h, w, H, W);
  else hipLaunchKernelGGL(upsample_argmax_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, labels, gt, counts, frames, nc, h, w, H, W);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// segcata/cata_test.py:115-170 + utils/cata_metrics.py: F.interpolate(out, (H, W), bilinear, align_corners) -> argmax, then one
// confusion matrix over the whole test set (rows gt, columns prediction; a pixel counts only when both lie in [0, ncm)).  Each block
// takes UA_CM_PIX consecutive output pixels of one frame, counts its pixels into an LDS histogram of ncm x ncm int32 bins and adds
// every non-zero bin to the caller's 64-bit matrix with one atomic: integer adds only, so the matrix does not depend on the order.
// align_corners = 0 is ATen's area_pixel_compute_source_index: src = max(scale (dst + 0.5) - 0.5, 0), scale = in / out.
#define UA_CM_PIX 1024

template <typename TL, bool CM>
__global__ __launch_bounds__(256) void upsample_argmax_cm_kernel(const TL* __restrict__ logits, unsigned char* __restrict__ labels,
                                                                 const long* __restrict__ gt, unsigned long long* cm, int ncm,
                                                                 int align, int nc, int h, int w, int H, int W) {
  __shared__ int hist[CM ? 64 * 64 : 1];
  const int bins = ncm * ncm;
  if (CM) {
    for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    __syncthreads();
  }
  const long per_frame = (long)H * W;
  const long blocks_per_frame = (per_frame + UA_CM_PIX - 1) / UA_CM_PIX;
  const int f = (int)(blockIdx.x / blocks_per_frame);
  const long p0 = (blockIdx.x % blocks_per_frame) * UA_CM_PIX;
  const float sy = align ? (H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f) : (float)h / (float)H;
  const float sx = align ? (W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f) : (float)w / (float)W;
  const TL* b = logits + (long)f * nc * h * w;
  for (int k = 0; k < UA_CM_PIX / 256; ++k) {
    const long px = p0 + k * 256 + threadIdx.x;
    if (px >= per_frame) break;
    const int x = (int)(px % W), y = (int)(px / W);
    float fy, fx;
    if (align) {
      fy = y * sy;
      fx = x * sx;
    } else {
      fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f);
      fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
    }
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float wy = fy - y0, wx = fx - x0;
    float best = -3.0e38f; int arg = 0;
    for (int c = 0; c < nc; ++c) {
      const TL* pl = b + (long)c * h * w;
      const float v = (1.f - wy) * ((1.f - wx) * to_f32<TL>(pl[y0 * w + x0]) + wx * to_f32<TL>(pl[y0 * w + x1])) +
                      wy * ((1.f - wx) * to_f32<TL>(pl[y1 * w + x0]) + wx * to_f32<TL>(pl[y1 * w + x1]));
      if (v > best) { best = v; arg = c; }
    }
    if (labels) labels[(long)f * per_frame + px] = (unsigned char)arg;
    if (CM) {
      const long g = gt[(long)f * per_frame + px];
      if (g >= 0 && g < ncm && arg < ncm) atomicAdd(&hist[(int)g * ncm + arg], 1);
    }
  }
  if (CM) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
      if (hist[i]) atomicAdd(cm + i, (unsigned long long)hist[i]);
  }
}

extern "C" int stswin_upsample_argmax_cm(int dtype, const void* logits, unsigned char* labels, const long* gt, unsigned long long* cm,
                                         int ncm, int align_corners, int frames, int nc, int h, int w, int H, int W, void* stream) {
  if (nc <= 0 || nc > 64 || frames <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return -1406;
  if (logits == nullptr) return -1407;
  const bool with_cm = gt != nullptr || cm != nullptr;
  if (with_cm && (gt == nullptr || cm == nullptr || ncm <= 0 || ncm > 64)) return -1408;
  if (!with_cm && labels == nullptr) return -1409;                  // nothing to write
  const long bpf = ((long)H * W + UA_CM_PIX - 1) / UA_CM_PIX;
  dim3 grid((unsigned)(bpf * frames));
  hipStream_t st = (hipStream_t)stream;
  const int al = align_corners ? 1 : 0;
  if (dtype == 0) {
    if (with_cm) hipLaunchKernelGGL((upsample_argmax_cm_kernel<bf16, true>), grid, dim3(256), 0, st, (const bf16*)logits, labels, gt, cm, ncm, al, nc, h, w, H, W);
    else hipLaunchKernelGGL((upsample_argmax_cm_kernel<bf16, false>), grid, dim3(256), 0, st, (const bf16*)logits, labels, gt, cm, ncm, al, nc, h, w, H, W);
  } else {
    if (with_cm) hipLaunchKernelGGL((upsample_argmax_cm_kernel<float, true>), grid, dim3(256), 0, st, (const float*)logits, labels, gt, cm, ncm, al, nc, h, w, H, W);
    else hipLaunchKernelGGL((upsample_argmax_cm_kernel<float, false>), grid, dim3(256), 0, st, (const float*)logits, labels, gt, cm, ncm, al, nc, h, w, H, W);
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Colour overlay of a label map (the picture seg18/test.py:162-169 and segcata/utils/cadis_visualization.py:86-113 make on the host):
// out = (a c + (255 - a) s + 127) / 255 per channel, (c, a) = table[label], s = the frame byte (0 without frames); a pixel whose label
// differs from a left / right / upper / lower neighbour of its own frame takes a = edge_alpha (>= 0).  One pass over 7 bytes per pixel.
// The pixels of all frames are one flat run p = (f H + y) W + x.  The wide body gives a thread OV_PPT = 8 consecutive pixels: one
// 8-byte label load, three 8-byte frame loads, three 8-byte stores (3 * 8 p is a multiple of 8), so it needs labels, frames and out
// 8-byte aligned and nothing of W: a group may straddle rows and frames, x and y are carried per pixel.  The rows above and below are
// read as 8 unaligned bytes each and the two flat neighbours of the group as single bytes, all through the cache (the same lines the
// neighbouring threads load as their own labels); a neighbour that does not exist is never compared, so what is loaded for it does not
// matter, but no load leaves [0, N).  The last N % 8 pixels, and every pixel when a pointer is not 8-byte aligned, take the byte body.
// The table goes to LDS byte by byte (any alignment) as r | g << 8 | b << 16 | a << 24.
#define OV_PPT 8

template <typename IT>
__device__ __forceinline__ void overlay_pixel(const unsigned char* labels, const unsigned char* frames, const unsigned* tab,
                                              unsigned char* out, IT p, int H, int W, int edge_alpha) {
  const unsigned l = labels[p];
  const unsigned e = tab[l];
  unsigned a = e >> 24;
  if (edge_alpha >= 0) {
    const IT row = p / (IT)W;
    const int x = (int)(p - row * (IT)W), y = (int)(row % (IT)H);
    const bool edge = (x > 0 && labels[p - 1] != l) || (x < W - 1 && labels[p + 1] != l) ||
                      (y > 0 && labels[p - (IT)W] != l) || (y < H - 1 && labels[p + (IT)W] != l);
    if (edge) a = (unsigned)edge_alpha;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned s = frames ? frames[3 * p + c] : 0u;
    out[3 * p + c] = (unsigned char)((a * ((e >> (8 * c)) & 255u) + (255u - a) * s + 127u) / 255u);
  }
}

__device__ __forceinline__ void overlay_load_table(const unsigned char* table, unsigned* tab) {
  const unsigned char* t = table + 4 * threadIdx.x;            // 256 threads, 256 entries
  tab[threadIdx.x] = (unsigned)t[0] | ((unsigned)t[1] << 8) | ((unsigned)t[2] << 16) | ((unsigned)t[3] << 24);
  __syncthreads();
}

template <typename IT>
__global__ __launch_bounds__(256) void labels_overlay_wide_kernel(const unsigned char* labels, const unsigned char* frames,
                                                                  const unsigned char* table, unsigned char* out, IT N, int H, int W,
                                                                  int edge_alpha) {
  __shared__ unsigned tab[256];
  overlay_load_table(table, tab);
  const IT p = ((IT)blockIdx.x * 256 + threadIdx.x) * OV_PPT;
  if (p >= N) return;
  if (p + OV_PPT > N) {                                        // the one partial group
    for (IT q = p; q < N; ++q) overlay_pixel<IT>(labels, frames, tab, out, q, H, W, edge_alpha);
    return;
  }
  const uint2 lw = *reinterpret_cast<const uint2*>(labels + p);
  unsigned l[OV_PPT], a[OV_PPT], e[OV_PPT];
#pragma unroll
  for (int i = 0; i < OV_PPT; ++i) {
    l[i] = ((i < 4 ? lw.x : lw.y) >> (8 * (i & 3))) & 255u;
    e[i] = tab[l[i]];
    a[i] = e[i] >> 24;
  }
  if (edge_alpha >= 0) {
    uint2 uw = make_uint2(0u, 0u), dw = make_uint2(0u, 0u);
    if (p >= (IT)W) {
      __builtin_memcpy(&uw, labels + (p - (IT)W), 8);
    } else {                                                   // frame 0, row 0 (and the start of row 1 when W < 8)
      unsigned long long v = 0;
      for (int i = 0; i < OV_PPT; ++i)
        if (p + i >= (IT)W) v |= (unsigned long long)labels[p + i - (IT)W] << (8 * i);
      uw = make_uint2((unsigned)v, (unsigned)(v >> 32));
    }
    if (p + (IT)W + OV_PPT <= N) {
      __builtin_memcpy(&dw, labels + (p + (IT)W), 8);
    } else {                                                   // the last row of the last frame
      unsigned long long v = 0;
      for (int i = 0; i < OV_PPT; ++i)
        if (p + i + (IT)W < N) v |= (unsigned long long)labels[p + i + (IT)W] << (8 * i);
      dw = make_uint2((unsigned)v, (unsigned)(v >> 32));
    }
    const unsigned left = p > 0 ? labels[p - 1] : 0u, right = p + OV_PPT < N ? labels[p + OV_PPT] : 0u;
    const IT row = p / (IT)W;
    int x = (int)(p - row * (IT)W), y = (int)(row % (IT)H);
#pragma unroll
    for (int i = 0; i < OV_PPT; ++i) {
      const unsigned up = ((i < 4 ? uw.x : uw.y) >> (8 * (i & 3))) & 255u, dn = ((i < 4 ? dw.x : dw.y) >> (8 * (i & 3))) & 255u;
      const unsigned lf = i ? l[i ? i - 1 : 0] : left, rt = i < OV_PPT - 1 ? l[i < OV_PPT - 1 ? i + 1 : 0] : right;
      const bool edge = (x > 0 && lf != l[i]) || (x < W - 1 && rt != l[i]) || (y > 0 && up != l[i]) || (y < H - 1 && dn != l[i]);
      if (edge) a[i] = (unsigned)edge_alpha;
      if (++x == W) {
        x = 0;
        if (++y == H) y = 0;
      }
    }
  }
  unsigned s[6] = {0u, 0u, 0u, 0u, 0u, 0u};                    // 24 frame bytes
  if (frames) {
    const uint2* fp = reinterpret_cast<const uint2*>(frames + 3 * p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint2 v = fp[k];
      s[2 * k] = v.x;
      s[2 * k + 1] = v.y;
    }
  }
  unsigned o[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 3 * OV_PPT; ++j) {
    const int i = j / 3, c = j % 3;
    const unsigned sb = (s[j >> 2] >> (8 * (j & 3))) & 255u;
    o[j >> 2] |= ((a[i] * ((e[i] >> (8 * c)) & 255u) + (255u - a[i]) * sb + 127u) / 255u) << (8 * (j & 3));
  }
  uint2* op = reinterpret_cast<uint2*>(out + 3 * p);
#pragma unroll
  for (int k = 0; k < 3; ++k) op[k] = make_uint2(o[2 * k], o[2 * k + 1]);
}

template <typename IT>
__global__ __launch_bounds__(256) void labels_overlay_byte_kernel(const unsigned char* labels, const unsigned char* frames,
                                                                  const unsigned char* table, unsigned char* out, IT N, int H, int W,
                                                                  int edge_alpha) {
  __shared__ unsigned tab[256];
  overlay_load_table(table, tab);
  const IT p = (IT)blockIdx.x * 256 + threadIdx.x;
  if (p < N) overlay_pixel<IT>(labels, frames, tab, out, p, H, W, edge_alpha);
}

extern "C" int stswin_labels_overlay(const unsigned char* labels, const unsigned char* frames, const unsigned char* table,
                                     unsigned char* out, int n, int H, int W, int edge_alpha, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0) return -1415;
  if (labels == nullptr || table == nullptr || out == nullptr) return -1416;
  if (edge_alpha < -1 || edge_alpha > 255) return -1417;
  const long N = (long)n * H * W;
  const bool wide = (((uintptr_t)labels | (uintptr_t)frames | (uintptr_t)out) & 7) == 0;
  const bool small = 3 * N + OV_PPT + W < (1L << 31);        // every index the kernels form fits 32 bits
  const long threads = wide ? (N + OV_PPT - 1) / OV_PPT : N;
  const long blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffL) return -1415;
  dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  if (wide) {
    if (small) hipLaunchKernelGGL(labels_overlay_wide_kernel<unsigned>, grid, dim3(256), 0, st, labels, frames, table, out, (unsigned)N, H, W, edge_alpha);
    else hipLaunchKernelGGL(labels_overlay_wide_kernel<long>, grid, dim3(256), 0, st, labels, frames, table, out, N, H, W, edge_alpha);
  } else {
    if (small) hipLaunchKernelGGL(labels_overlay_byte_kernel<unsigned>, grid, dim3(256), 0, st, labels, frames, table, out, (unsigned)N, H, W, edge_alpha);
    else hipLaunchKernelGGL(labels_overlay_byte_kernel<long>, grid, dim3(256), 0, st, labels, frames, table, out, N, H, W, edge_alpha);
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Ground truth as the files hold it -> class indices (what seg18/dataset/Endovis2018_new.py:130-136 and segcata/dataset/
// CATA_new_512.py:97, 237 do on the host).  CH = 3 | 4: the pixel's (r, g, b) is looked up in a table of up to 256 rows (r, g, b,
// label), the last equal row wins, none gives 0 and counts the pixel as unmatched; CH = 1: out = table[u].  The table sits in LDS, a
// colour row as r | g << 8 | b << 16 | label << 24, so the search is one broadcast LDS read per row and a compare per pixel.  The
// pixels of all frames are one flat run.  The wide body gives a thread GT_PPT = 4 consecutive pixels: 16 bytes of RGBA, three dwords
// of RGB or one dword of ids in, one dword of uint8 or two 16-byte stores of int64 out, so it needs `in` 16-byte (RGBA) or 4-byte
// aligned and `out` 4-byte (uint8) or 16-byte (int64) aligned, and nothing of W or H * W; the last N % 4 pixels, and every pixel when
// a pointer is not so aligned, go byte by byte.  Unmatched pixels: a workgroup counts those of the frame its first pixel lies in
// in LDS and adds them with one atomic if there are any; a pixel of a later frame (a workgroup that straddles a frame border)
// adds itself.
#define GT_PPT 4

template <int CH, typename OT, typename IT, bool WIDE>
__global__ __launch_bounds__(256) void gt_decode_kernel(const unsigned char* in, const unsigned char* table, OT* out, int* unmatched,
                                                        IT N, IT HW, int ncolours) {
  constexpr int PPT = WIDE ? GT_PPT : 1;
  __shared__ unsigned tab[256];
  __shared__ int missed;
  if (CH == 1) {
    tab[threadIdx.x] = table[threadIdx.x];                     // 256 threads, 256 entries
  } else if ((int)threadIdx.x < ncolours) {
    const unsigned char* t = table + 4 * threadIdx.x;          // byte by byte: any alignment
    tab[threadIdx.x] = (unsigned)t[0] | ((unsigned)t[1] << 8) | ((unsigned)t[2] << 16) | ((unsigned)t[3] << 24);
  }
  if (threadIdx.x == 0) missed = 0;
  __syncthreads();
  const IT first = (IT)blockIdx.x * (256 * PPT);               // the workgroup's first pixel (< N: the grid is ceil(N / (256 PPT)))
  const IT p = first + (IT)threadIdx.x * PPT;
  const int cnt = p >= N ? 0 : (N - p >= (IT)PPT ? PPT : (int)(N - p));
  unsigned k[PPT], lab[PPT];
  bool miss[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) k[j] = 0u;
  if (WIDE && cnt == PPT) {
    if (CH == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(in + 4 * p);
      k[0] = v.x & 0xffffffu;
      k[1 % PPT] = v.y & 0xffffffu;
      k[2 % PPT] = v.z & 0xffffffu;
      k[3 % PPT] = v.w & 0xffffffu;
    } else if (CH == 3) {
      const unsigned* w = reinterpret_cast<const unsigned*>(in + 3 * p);
      const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
      k[0] = w0 & 0xffffffu;
      k[1 % PPT] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
      k[2 % PPT] = (w1 >> 16) | ((w2 & 0xffu) << 16);
      k[3 % PPT] = w2 >> 8;
    } else {
      const unsigned w = *reinterpret_cast<const unsigned*>(in + p);
#pragma unroll
      for (int j = 0; j < PPT; ++j) k[j] = (w >> (8 * j)) & 255u;
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      if (j < cnt) {
        const unsigned char* s = in + (IT)CH * (p + j);
        k[j] = CH == 1 ? (unsigned)s[0] : ((unsigned)s[0] | ((unsigned)s[1 % CH] << 8) | ((unsigned)s[2 % CH] << 16));
      }
    }
  }
  if (CH == 1) {
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      lab[j] = tab[k[j]];
      miss[j] = false;
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      lab[j] = 0u;
      miss[j] = true;
    }
    for (int i = 0; i < ncolours; ++i) {                       // rows in order: a later equal row overwrites
      const unsigned e = tab[i];
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        if ((e & 0xffffffu) == k[j]) {
          lab[j] = e >> 24;
          miss[j] = false;
        }
      }
    }
  }
  if (WIDE && cnt == PPT) {
    if (sizeof(OT) == 1) {
      *reinterpret_cast<unsigned*>(out + p) = lab[0] | (lab[1 % PPT] << 8) | (lab[2 % PPT] << 16) | (lab[3 % PPT] << 24);
    } else {
      uint4* o = reinterpret_cast<uint4*>(out + p);
      o[0] = make_uint4(lab[0], 0u, lab[1 % PPT], 0u);
      o[1] = make_uint4(lab[2 % PPT], 0u, lab[3 % PPT], 0u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPT; ++j)
      if (j < cnt) out[p + j] = (OT)lab[j];
  }
  if (CH != 1 && unmatched != nullptr) {                       // (uniform: no thread has left the kernel)
    const IT f0 = first / HW;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      if (j < cnt && miss[j]) {
        const IT f = (p + j) / HW;
        if (f == f0) ++mine;
        else atomicAdd(unmatched + f, 1);
      }
    }
    if (mine) atomicAdd(&missed, mine);
    __syncthreads();
    if (threadIdx.x == 0 && missed) atomicAdd(unmatched + f0, missed);
  }
}

template <int CH, typename OT>
static void gt_decode_launch(const unsigned char* in, const unsigned char* table, void* out, int* unmatched, long N, long HW, int ncolours,
                             bool wide, bool small, dim3 grid, hipStream_t st) {
  OT* o = (OT*)out;
  if (wide) {
    if (small) hipLaunchKernelGGL((gt_decode_kernel<CH, OT, unsigned, true>), grid, dim3(256), 0, st, in, table, o, unmatched, (unsigned)N, (unsigned)HW, ncolours);
    else hipLaunchKernelGGL((gt_decode_kernel<CH, OT, long, true>), grid, dim3(256), 0, st, in, table, o, unmatched, N, HW, ncolours);
  } else {
    if (small) hipLaunchKernelGGL((gt_decode_kernel<CH, OT, unsigned, false>), grid, dim3(256), 0, st, in, table, o, unmatched, (unsigned)N, (unsigned)HW, ncolours);
    else hipLaunchKernelGGL((gt_decode_kernel<CH, OT, long, false>), grid, dim3(256), 0, st, in, table, o, unmatched, N, HW, ncolours);
  }
}

extern "C" int stswin_gt_decode(const unsigned char* in, const unsigned char* table, void* out, int* unmatched, int n, int H, int W,
                                int ch, int ncolours, int out_bytes, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0) return -1418;
  if (in == nullptr || table == nullptr || out == nullptr) return -1419;
  if (ch != 1 && ch != 3 && ch != 4) return -1420;
  if (ncolours < 1 || ncolours > 256) return -1421;
  if (out_bytes != 1 && out_bytes != 8) return -1422;
  const long HW = (long)H * W, N = (long)n * HW;
  const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
  if (i0 < o0 + (uintptr_t)(N * out_bytes) && o0 < i0 + (uintptr_t)(N * ch)) return -1423;
  const bool wide = (i0 & (ch == 4 ? 15 : 3)) == 0 && (o0 & (out_bytes == 8 ? 15 : 3)) == 0;
  const bool small = 4 * N + 256 * GT_PPT < (1L << 31);        // every index the kernels form fits 32 bits
  const long per = 256L * (wide ? GT_PPT : 1);
  const long blocks = (N + per - 1) / per;
  if (blocks > 0x7fffffffL) return -1418;
  dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
#define GT_LAUNCH(CH_)                                                                                                      \
  do {                                                                                                                      \
    if (out_bytes == 8) gt_decode_launch<CH_, long>(in, table, out, unmatched, N, HW, ncolours, wide, small, grid, st); \
    else gt_decode_launch<CH_, unsigned char>(in, table, out, unmatched, N, HW, ncolours, wide, small, grid, st);         \
  } while (0)
  if (ch == 1) GT_LAUNCH(1);
  else if (ch == 3) GT_LAUNCH(3);
  else GT_LAUNCH(4);
#undef GT_LAUNCH
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Per-frame, per-class moments of a label map (stswincl_amd/utils/instruments.py states the row; VideoSegmenter(report=...)): count,
// sum x, sum y, sum x^2, sum xy, sum y^2 and the extent as four maxima, over the pixels of each label < nc.  One pass over 1 byte per
// pixel.  A thread takes ONE chunk of up to 16 pixels of one row (the wide body: one 16-byte load, which needs labels 16-byte aligned
// and W % 16 == 0 so that every row of every frame starts on the grid; otherwise 16 byte loads and the row's last chunk is short); a
// workgroup of LM_THREADS = 512 threads takes 512 consecutive chunks (8 KB) of ONE frame, a wave 64 consecutive ones.
//   * A full chunk of one label (label maps are long runs: nearly every chunk) is the six small numbers 1, cx, dy, cx^2, cx dy, dy^2
//     with cx = x0 / 16 its chunk column and dy its row less the row of the wave's first chunk.  Per distinct label among the wave's
//     such chunks these are summed across the wave in 32 bits (six DPP steps per number, no LDS traffic), the extent comes from the
//     first and last lane (rows) and two more DPP maxima (columns), and lane 63 alone expands the sums to the ten terms in 64 bits -
//     sum_{i<16} (16 cx + i) = 256 cx + 120, sum (16 cx + i)^2 = 4096 cx^2 + 3840 cx + 1240 - and adds them to the workgroup's LDS table.
//   * A chunk with several runs, or a short one, adds run by run: a run [first, last] of row y is n, n (first + last) / 2,
//     n first^2 + 2 first T1 + T2 with T1, T2 the sums of i and i^2 below n, and y n, y sum x, y^2 n.
// At the end the workgroup adds its non-zero LDS entries to out[f] with 64-bit global atomics: integer adds and maxima only, so the
// result is exact and does not depend on the order.  The workgroup size is measured, not derived ("Instrument report"): on a
// cold map the launch costs 1.3 us per 4 KB that ONE workgroup reads, whatever the code does with them, and 16 ns per workgroup of the
// frame, because all of them queue up on the background's ten entries of out; 8 KB per workgroup is where the two meet at 1024 x 1280.
#define LM_THREADS 512

struct LmTerms {
  unsigned n, sx, sy;                  // < 2^32 for one run and for a wave's 64 chunks (64 * 16 * 16383)
  unsigned long long sxx, sxy, syy;
  unsigned e0, e1, e2, e3;             // W - first, H - y, last + 1, y + 1
};

__device__ __forceinline__ LmTerms lm_run(unsigned first, unsigned n, unsigned y, unsigned H, unsigned W) {
  LmTerms t;
  const unsigned last = first + n - 1;
  const unsigned t1 = n * (n - 1) / 2, t2 = (n - 1) * n * (2 * n - 1) / 6;
  t.n = n;
  t.sx = n * (first + last) / 2;
  t.sy = y * n;
  t.sxx = (unsigned long long)(first * first) * n + (unsigned long long)(2 * first * t1 + t2);
  t.sxy = (unsigned long long)y * t.sx;
  t.syy = (unsigned long long)(y * y) * n;
  t.e0 = W - first;
  t.e1 = H - y;
  t.e2 = last + 1;
  t.e3 = y + 1;
  return t;
}

__device__ __forceinline__ void lm_flush(unsigned long long* sums, unsigned* ext, unsigned l, const LmTerms& t) {
  unsigned long long* s = sums + 6 * l;
  atomicAdd(s + 0, (unsigned long long)t.n);
  atomicAdd(s + 1, (unsigned long long)t.sx);
  atomicAdd(s + 2, (unsigned long long)t.sy);
  atomicAdd(s + 3, t.sxx);
  atomicAdd(s + 4, t.sxy);
  atomicAdd(s + 5, t.syy);
  unsigned* e = ext + 4 * l;
  atomicMax(e + 0, t.e0);
  atomicMax(e + 1, t.e1);
  atomicMax(e + 2, t.e2);
  atomicMax(e + 3, t.e3);
}

__device__ __forceinline__ unsigned lm_byte(const uint4& v, int i) {          // (i is a constant or selects by compares: no indexing)
  return ((i < 4 ? v.x : i < 8 ? v.y : i < 12 ? v.z : v.w) >> (8 * (i & 3))) & 255u;
}

// The wave's sum / maximum of an unsigned value, valid in lane 63; every lane of the wave must be active.  quad_perm [1,0,3,2] and
// [2,3,0,1], row_shr 4 and 8 leave a row's total in its lane 15; row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3 carry
// the totals on.  A lane without a source reads 0, the identity of both operations.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned lm_dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}

template <bool MAX>
__device__ __forceinline__ unsigned lm_wave(unsigned v) {
#define LM_STEP(CTRL, ROWS)                          \
  {                                                  \
    const unsigned o = lm_dpp<CTRL, ROWS>(v);        \
    v = MAX ? max(v, o) : v + o;                     \
  }
  LM_STEP(0xb1, 0xf)
  LM_STEP(0x4e, 0xf)
  LM_STEP(0x114, 0xf)
  LM_STEP(0x118, 0xf)
  LM_STEP(0x142, 0xa)
  LM_STEP(0x143, 0xc)
#undef LM_STEP
  return v;
}

template <bool WIDE>
__global__ __launch_bounds__(LM_THREADS) void label_moments_kernel(const unsigned char* __restrict__ labels, unsigned long long* out, int H,
                                                                   int W, int nc, int cpr, int blocks_per_frame) {
  __shared__ unsigned long long sums[64 * 6];
  __shared__ unsigned ext[64 * 4];
  for (int i = threadIdx.x; i < 6 * nc; i += LM_THREADS) sums[i] = 0ull;
  for (int i = threadIdx.x; i < 4 * nc; i += LM_THREADS) ext[i] = 0u;
  __syncthreads();
  const int f = (int)(blockIdx.x / (unsigned)blocks_per_frame);
  const int q = (int)(blockIdx.x % (unsigned)blocks_per_frame) * LM_THREADS + (int)threadIdx.x;      // < 2^24 + 2^10 chunks of the frame
  const int row = q / cpr, col = q - row * cpr;
  const bool valid = row < H;                                  // (the chunk exists; the wave's lanes with a chunk are a prefix)
  const int len = valid ? min(16, W - 16 * col) : 0;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (valid) {
    const unsigned char* p = labels + ((long)f * H + row) * W + 16 * col;
    if (WIDE) {
      v = *reinterpret_cast<const uint4*>(p);
    } else {
      unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < len) w[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  const unsigned l0 = v.x & 255u, splat = l0 * 0x01010101u;
  const bool full = len == 16 && v.x == splat && v.y == splat && v.z == splat && v.w == splat;       // the usual chunk: one label
  if (valid && !full) {
    unsigned change = 0;               // bit i: pixel i starts a run (i >= 1)
#pragma unroll
    for (int i = 1; i < 16; ++i)
      if (lm_byte(v, i) != lm_byte(v, i - 1)) change |= 1u << i;
    change &= (1u << len) - 1u;
    int a = 0;
    while (a < len) {
      const unsigned rest = change >> (a + 1);
      const int e = rest ? a + 1 + __builtin_ctz(rest) : len;
      const unsigned l = lm_byte(v, a);
      if (l < (unsigned)nc) lm_flush(sums, ext, l, lm_run((unsigned)(16 * col + a), (unsigned)(e - a), (unsigned)row, (unsigned)H, (unsigned)W));
      a = e;
    }
  }
  // the full chunks, label by label (wave-uniform from here: every lane takes part in the sums)
  const unsigned row_w = (unsigned)__builtin_amdgcn_readfirstlane(row);       // lane 0's row: the smallest of the wave
  const unsigned cx = (unsigned)col, dy = (unsigned)row - row_w;              // dy <= 64 / cpr + 1
  unsigned long long todo = __ballot(full && l0 < (unsigned)nc);
  while (todo) {
    const int first = __ffsll((long long)todo) - 1;
    const unsigned L = (unsigned)__builtin_amdgcn_readlane((int)l0, first);
    const bool mine = full && l0 == L;
    const unsigned long long m = __ballot(mine);
    todo &= ~m;
    const int last = 63 - __clzll((long long)m);
    const unsigned mcx = mine ? cx : 0u, mdy = mine ? dy : 0u;
    // <= 64 lanes of cx < 1024, dy <= 65: every sum stays far below 2^32; the count and sum dy share a word (64 < 2^8)
    const unsigned c_sdy = lm_wave<false>((mine ? 1u : 0u) | (mdy << 8));
    const unsigned scx = lm_wave<false>(mcx), scx2 = lm_wave<false>(mcx * mcx), scxdy = lm_wave<false>(mcx * mdy);
    const unsigned sdy2 = lm_wave<false>(mdy * mdy);
    const unsigned cx_max = lm_wave<true>(mcx), cx_min = 1023u - lm_wave<true>(mine ? 1023u - cx : 0u);
    const unsigned dy_min = (unsigned)__builtin_amdgcn_readlane((int)dy, first), dy_max = (unsigned)__builtin_amdgcn_readlane((int)dy, last);
    if ((threadIdx.x & 63) == 63) {
      const unsigned c = c_sdy & 255u, sdy = c_sdy >> 8;
      const unsigned sy = c * row_w + sdy;                                                      // sum of the chunks' rows
      const unsigned long long scxy = (unsigned long long)row_w * scx + scxdy;
      const unsigned long long sy2 = (unsigned long long)c * (row_w * row_w) + (unsigned long long)(2u * row_w * sdy + sdy2);
      LmTerms t;
      t.n = 16u * c;
      t.sx = 256u * scx + 120u * c;
      t.sy = 16u * sy;
      t.sxx = 4096ull * scx2 + (unsigned long long)(3840u * scx + 1240u * c);
      t.sxy = 256ull * scxy + 120ull * sy;
      t.syy = 16ull * sy2;
      t.e0 = (unsigned)W - 16u * cx_min;
      t.e1 = (unsigned)H - (row_w + dy_min);
      t.e2 = 16u * cx_max + 16u;
      t.e3 = row_w + dy_max + 1u;
      lm_flush(sums, ext, L, t);
    }
  }
  __syncthreads();
  unsigned long long* o = out + (long)f * nc * 10;
  for (int i = threadIdx.x; i < 10 * nc; i += LM_THREADS) {
    const int c = i / 10, k = i - 10 * c;
    if (k < 6) {
      const unsigned long long s = sums[6 * c + k];
      if (s) atomicAdd(o + i, s);
    } else {
      const unsigned e = ext[4 * c + k - 6];
      if (e) atomicMax(o + i, (unsigned long long)e);
    }
  }
}

extern "C" int stswin_label_moments(const unsigned char* labels, long long* out, int n, int H, int W, int nc, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1545;
  if (labels == nullptr || out == nullptr) return -1546;
  if (nc < 1 || nc > 64) return -1547;
  const bool wide = ((uintptr_t)labels & 15) == 0 && W % 16 == 0;
  const int cpr = (W + 15) / 16;
  const long chunks = (long)H * cpr;
  const long bpf = (chunks + LM_THREADS - 1) / LM_THREADS;
  if (bpf * n > 0x7fffffffL) return -1545;
  dim3 grid((unsigned)(bpf * n));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  if (wide) hipLaunchKernelGGL(label_moments_kernel<true>, grid, dim3(LM_THREADS), 0, st, labels, o, H, W, nc, cpr, (int)bpf);
  else hipLaunchKernelGGL(label_moments_kernel<false>, grid, dim3(LM_THREADS), 0, st, labels, o, H, W, nc, cpr, (int)bpf);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Confidence of the labels (stswincl_amd/utils/confidence.py states the result; VideoSegmenter(confidence=...)): the softmax
// probability seg18/test.py:153-158 has between its resize and its argmax, for the label a pixel got, as a byte.  The label launches
// above skip the softmax, so this launch reads the small logits once more: a thread takes CF_PPT = 4 pixels of one output row, which
// share y0, y1 and wy, with the coordinate and value expressions of upsample_argmax_kernel / upsample_argmax_cm_kernel copied to the
// letter (this file is built with -ffp-contract=off), so the value at a label those kernels made is the running maximum to the bit.
// The softmax is online - per class one expf of -|v - m| rescales the sum or joins it - so nothing is indexed by the class: no scratch.
// WIDE: labels and conf 4-byte aligned and W % 4 == 0, one dword in and out; else the bytes that exist, one by one.
#define CF_PPT 4

template <typename TL, bool WIDE>
__global__ __launch_bounds__(256) void upsample_confidence_kernel(const TL* __restrict__ logits, const unsigned char* __restrict__ labels,
                                                                  unsigned char* __restrict__ conf, int align, int nc, int h, int w, int H,
                                                                  int W, int cpr, int blocks_per_frame) {
  const int f = (int)(blockIdx.x / (unsigned)blocks_per_frame);
  const long q = (long)(blockIdx.x % (unsigned)blocks_per_frame) * 256 + threadIdx.x;
  const int y = (int)(q / cpr), col = (int)(q - (long)y * cpr);
  if (y >= H) return;
  const int xb = CF_PPT * col, len = min(CF_PPT, W - xb);
  const long at = ((long)f * H + y) * W + xb;
  unsigned lw = 0u;
  if (WIDE) {
    lw = *reinterpret_cast<const unsigned*>(labels + at);
  } else {
#pragma unroll
    for (int i = 0; i < CF_PPT; ++i)
      if (i < len) lw |= (unsigned)labels[at + i] << (8 * i);
  }
  const float sy = align ? (H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f) : (float)h / (float)H;
  const float sx = align ? (W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f) : (float)w / (float)W;
  float fy;
  if (align) fy = y * sy;
  else fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f);
  const int y0 = min((int)fy, h - 1);
  const int y1 = min(y0 + 1, h - 1);
  const float wy = fy - y0;
  int x0[CF_PPT], x1[CF_PPT];
  float wx[CF_PPT], m[CF_PPT], s[CF_PPT], vl[CF_PPT];
#pragma unroll
  for (int i = 0; i < CF_PPT; ++i) {
    const int x = min(xb + i, W - 1);                          // (a pixel past the row's end repeats the last one and is not stored)
    float fx;
    if (align) fx = x * sx;
    else fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
    x0[i] = min((int)fx, w - 1);
    x1[i] = min(x0[i] + 1, w - 1);
    wx[i] = fx - x0[i];
    m[i] = -3.0e38f;
    s[i] = 0.f;
    vl[i] = 0.f;
  }
  const TL* b = logits + (long)f * nc * h * w;
  for (int c = 0; c < nc; ++c) {
    const TL* pl = b + (long)c * h * w;
    const TL* r0 = pl + y0 * w;
    const TL* r1 = pl + y1 * w;
#pragma unroll
    for (int i = 0; i < CF_PPT; ++i) {
      const float v = (1.f - wy) * ((1.f - wx[i]) * to_f32<TL>(r0[x0[i]]) + wx[i] * to_f32<TL>(r0[x1[i]])) +
                      wy * ((1.f - wx[i]) * to_f32<TL>(r1[x0[i]]) + wx[i] * to_f32<TL>(r1[x1[i]]));
      const float e = expf(-fabsf(v - m[i]));                  // v > m: the old sum's scale; else this class's term
      if (v > m[i]) {
        s[i] = s[i] * e + 1.f;
        m[i] = v;
      } else {
        s[i] += e;
      }
      if ((unsigned)c == ((lw >> (8 * i)) & 255u)) vl[i] = v;
    }
  }
  unsigned out = 0u;
#pragma unroll
  for (int i = 0; i < CF_PPT; ++i) {
    const unsigned l = (lw >> (8 * i)) & 255u;
    const float p = expf(vl[i] - m[i]) / s[i];
    const unsigned qv = l < (unsigned)nc ? (unsigned)fminf(255.f * p + 0.5f, 255.f) : 0u;
    out |= qv << (8 * i);
  }
  if (WIDE) {
    *reinterpret_cast<unsigned*>(conf + at) = out;
  } else {
#pragma unroll
    for (int i = 0; i < CF_PPT; ++i)
      if (i < len) conf[at + i] = (unsigned char)(out >> (8 * i));
  }
}

extern "C" int stswin_upsample_confidence(int dtype, const void* logits, const unsigned char* labels, unsigned char* conf,
                                          int align_corners, int frames, int nc, int h, int w, int H, int W, void* stream) {
  if (frames <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || (long)h * w > 0x7fffffffL) return -1880;
  if (nc < 1 || nc > 64) return -1881;
  if (logits == nullptr || labels == nullptr || conf == nullptr) return -1882;
  if (dtype != 0 && dtype != 1) return -1883;
  const bool wide = (((uintptr_t)labels | (uintptr_t)conf) & 3) == 0 && W % CF_PPT == 0;
  const int cpr = (W + CF_PPT - 1) / CF_PPT;
  const long bpf = ((long)H * cpr + 255) / 256;
  if (bpf * frames > 0x7fffffffL) return -1880;
  dim3 grid((unsigned)(bpf * frames));
  hipStream_t st = (hipStream_t)stream;
  const int al = align_corners ? 1 : 0;
#define CF_LAUNCH(TL, WIDE_)                                                                                                       \
  hipLaunchKernelGGL((upsample_confidence_kernel<TL, WIDE_>), grid, dim3(256), 0, st, (const TL*)logits, labels, conf, al, nc, h, w, \
                     H, W, cpr, (int)bpf)
  if (dtype == 0) {
    if (wide) CF_LAUNCH(bf16, true);
    else CF_LAUNCH(bf16, false);
  } else {
    if (wide) CF_LAUNCH(float, true);
    else CF_LAUNCH(float, false);
  }
#undef CF_LAUNCH
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Sums of the confidence map over a label map or a component map (utils/confidence.py, confidence_sums, states the result): per frame
// and map value i < K the number of pixels, the sum of their conf and the number with conf < low.  A workgroup takes CS_THREADS * 16
// consecutive pixels of one frame, a thread 16 of them; a thread adds a run of equal values to the workgroup's LDS bins at once (an
// instrument is spatially coherent: most threads flush once), and the non-zero bins go out with one 64-bit atomic each.  4096 pixels of
// conf <= 255 keep every bin below 2^21.  WIDE: 16-byte loads (the frame's pixels start 16-byte aligned); else element by element.
#define CS_THREADS 256
#define CS_PPT 16

__device__ __forceinline__ void cs_flush(unsigned* bins, int id, unsigned c, unsigned s, unsigned lo) {
  atomicAdd(bins + 3 * id, c);
  atomicAdd(bins + 3 * id + 1, s);
  if (lo) atomicAdd(bins + 3 * id + 2, lo);
}

template <int MB, bool WIDE>
__global__ __launch_bounds__(CS_THREADS) void confidence_sums_kernel(const void* __restrict__ map, const unsigned char* __restrict__ conf,
                                                                     unsigned long long* out, int K, unsigned low, long HW,
                                                                     int blocks_per_frame) {
  __shared__ unsigned bins[3 * 1024];
  for (int i = threadIdx.x; i < 3 * K; i += CS_THREADS) bins[i] = 0u;
  __syncthreads();
  const int f = (int)(blockIdx.x / (unsigned)blocks_per_frame);
  const long p0 = ((long)(blockIdx.x % (unsigned)blocks_per_frame) * CS_THREADS + threadIdx.x) * CS_PPT;
  const int len = (int)max(0L, min((long)CS_PPT, HW - p0));
  if (len > 0) {
    const long at = (long)f * HW + p0;
    int id[CS_PPT];
    unsigned qv[CS_PPT];
    if (WIDE) {                                                // (len == 16: H W % 16 == 0)
      const uint4 cw = *reinterpret_cast<const uint4*>(conf + at);
#pragma unroll
      for (int i = 0; i < CS_PPT; ++i) qv[i] = lm_byte(cw, i);
      if (MB == 1) {
        const uint4 mw = *reinterpret_cast<const uint4*>((const unsigned char*)map + at);
#pragma unroll
        for (int i = 0; i < CS_PPT; ++i) id[i] = (int)lm_byte(mw, i);
      } else {
        const int4* mp = reinterpret_cast<const int4*>((const int*)map + at);
#pragma unroll
        for (int k = 0; k < CS_PPT / 4; ++k) {
          const int4 mw = mp[k];
          id[4 * k] = mw.x;
          id[4 * k + 1] = mw.y;
          id[4 * k + 2] = mw.z;
          id[4 * k + 3] = mw.w;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < CS_PPT; ++i) {
        const bool in = i < len;
        qv[i] = in ? (unsigned)conf[at + i] : 0u;
        id[i] = !in ? -1 : MB == 1 ? (int)((const unsigned char*)map)[at + i] : ((const int*)map)[at + i];
      }
    }
    int cur = -1;
    unsigned c = 0u, s = 0u, lo = 0u;
#pragma unroll
    for (int i = 0; i < CS_PPT; ++i) {
      const int v = (unsigned)id[i] < (unsigned)K ? id[i] : -1;        // (-1, a value >= K and a pixel past the end: counted nowhere)
      if (v != cur) {
        if (cur >= 0) cs_flush(bins, cur, c, s, lo);
        cur = v;
        c = s = lo = 0u;
      }
      c += 1u;
      s += qv[i];
      lo += qv[i] < low ? 1u : 0u;
    }
    if (cur >= 0) cs_flush(bins, cur, c, s, lo);
  }
  __syncthreads();
  unsigned long long* o = out + (long)f * 3 * K;
  for (int i = threadIdx.x; i < 3 * K; i += CS_THREADS)
    if (bins[i]) atomicAdd(o + i, (unsigned long long)bins[i]);
}

extern "C" int stswin_confidence_sums(const void* map, int map_bytes, const unsigned char* conf, long long* out, int K, int low, int n,
                                      int H, int W, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1884;
  if (map == nullptr || conf == nullptr || out == nullptr) return -1885;
  if (map_bytes != 1 && map_bytes != 4) return -1886;
  if (K < 1 || K > 1024) return -1887;
  if (low < 0 || low > 256) return -1888;
  if (((uintptr_t)map & (uintptr_t)(map_bytes - 1)) || ((uintptr_t)out & 7)) return -1889;
  const long HW = (long)H * W;
  const long bpf = (HW + CS_THREADS * CS_PPT - 1) / (CS_THREADS * CS_PPT);
  if (bpf * n > 0x7fffffffL) return -1884;
  const bool wide = (((uintptr_t)map | (uintptr_t)conf) & 15) == 0 && HW % CS_PPT == 0;
  dim3 grid((unsigned)(bpf * n));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  stswin_zero_bytes(out, (size_t)n * K * 3 * sizeof(long long), st);        // (a kernel, not hipMemsetAsync: see common.h)
#define CS_LAUNCH(MB_, WIDE_)                                                                                                  \
  hipLaunchKernelGGL((confidence_sums_kernel<MB_, WIDE_>), grid, dim3(CS_THREADS), 0, st, map, conf, o, K, (unsigned)low, HW, \
                     (int)bpf)
  if (map_bytes == 1) {
    if (wide) CS_LAUNCH(1, true);
    else CS_LAUNCH(1, false);
  } else {
    if (wide) CS_LAUNCH(4, true);
    else CS_LAUNCH(4, false);
  }
#undef CS_LAUNCH
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Parts and contacts of the instances (utils/instruments.py, instance_parts, states the result; VideoSegmenter(parts=...)): per frame,
// instance ordinal i < K and class c < nc the ten integers of the moments row over the pixels with components == i and labels == c, and
// the number of pixel edges between instance i and pixels of class c outside it.  A workgroup takes a tile of IP_TH x IP_TW pixels of
// one frame, a thread IP_PPT = 16 consecutive pixels of one row.  A pixel becomes one word, (ordinal + 1) << 8 | label with ordinal + 1
// = 0 for -1 and ordinals >= K; the tile's words and those of the one-pixel frame around it (IP_NONE outside the map) go through LDS,
// so each map is read once plus that halo.  K nc 11 bins do not fit on chip, but a tile of a real map holds a handful of distinct
// (ordinal, class) keys: a thread folds the runs of equal keys along its 16 pixels in registers (the moments of a run in closed form
// by lm_run; the edges towards the row above, the row below, the left and the right each as runs of equal (ordinal, neighbour's
// class)) and adds every run to a keyed table of IP_SLOTS slots in LDS, found by a multiplicative hash and up to IP_PROBES linear
// probes.  The slots in use go out with one 64-bit atomic per non-zero integer.  A key that finds none of its probe slots free or its
// own - always so once the table is full - adds to the outputs directly: integer adds and maxima only, so the result is the same
// either way and whatever the order.  WIDE: both maps 16-byte aligned and W % 16 == 0, one 16-byte load of labels and four of
// components per thread; else element by element.  The halo is always read by element.
#define IP_TH 32
#define IP_TW 128
#define IP_PPT 16
#define IP_CPR (IP_TW / IP_PPT)               // threads per row of the tile
#define IP_THREADS (IP_TH * IP_CPR)
#define IP_RS (IP_TW + 4)                     // words per LDS row: 16-byte aligned rows that start on different banks
#define IP_SLOTS 64
#define IP_PROBES 8
#define IP_NONE 255u                          // no ordinal and a label no class has (nc <= 64): nobody's p, nobody's q
static_assert(IP_SLOTS == 64, "ip_slot takes the hash's top 6 bits");

struct IpTable {
  unsigned key[IP_SLOTS];                     // the slot's word (ordinal + 1) << 8 | class, 0: free
  unsigned long long sums[IP_SLOTS * 6];      // (a tile's sum x^2 passes 2^32)
  unsigned ext[IP_SLOTS * 4];
  unsigned touch[IP_SLOTS];                   // <= 4 IP_TH IP_TW
};

__device__ __forceinline__ unsigned ip_word(int comp, unsigned label, int K) {
  return ((unsigned)comp < (unsigned)K ? (unsigned)comp + 1u : 0u) << 8 | label;
}

__device__ __forceinline__ int ip_slot(IpTable& tb, unsigned word) {
  const unsigned h = (word * 2654435761u) >> 26;
  for (int t = 0; t < IP_PROBES; ++t) {
    const int s = (int)((h + t) & (IP_SLOTS - 1));
    const unsigned old = atomicCAS(&tb.key[s], 0u, word);
    if (old == 0u || old == word) return s;
  }
  return -1;
}

__device__ __forceinline__ long ip_at(unsigned word, int nc) { return (long)((word >> 8) - 1u) * nc + (long)(word & 255u); }

__device__ __forceinline__ void ip_moments(IpTable& tb, unsigned long long* parts_f, int nc, unsigned word, const LmTerms& t) {
  const int s = ip_slot(tb, word);
  if (s >= 0) {
    lm_flush(tb.sums, tb.ext, (unsigned)s, t);
  } else {
    unsigned long long* o = parts_f + ip_at(word, nc) * 10;
    atomicAdd(o + 0, (unsigned long long)t.n);
    atomicAdd(o + 1, (unsigned long long)t.sx);
    atomicAdd(o + 2, (unsigned long long)t.sy);
    atomicAdd(o + 3, t.sxx);
    atomicAdd(o + 4, t.sxy);
    atomicAdd(o + 5, t.syy);
    atomicMax(o + 6, (unsigned long long)t.e0);
    atomicMax(o + 7, (unsigned long long)t.e1);
    atomicMax(o + 8, (unsigned long long)t.e2);
    atomicMax(o + 9, (unsigned long long)t.e3);
  }
}

__device__ __forceinline__ void ip_touch(IpTable& tb, unsigned long long* contacts_f, int nc, unsigned word, unsigned edges) {
  const int s = ip_slot(tb, word);
  if (s >= 0) atomicAdd(&tb.touch[s], edges);
  else atomicAdd(contacts_f + ip_at(word, nc), (unsigned long long)edges);
}

// v[a] by masks: every element is read at a constant index (a chain of selects between the elements comes back from the compiler as
// one indexed load, and the array with it in scratch memory)
__device__ __forceinline__ unsigned ip_pick(const unsigned (&v)[IP_PPT], int a) {
  unsigned r = 0u;
#pragma unroll
  for (int k = 0; k < IP_PPT; ++k) r |= v[k] & (0u - (unsigned)(a == k));
  return r;
}

// f(word, first, length) for every run of equal non-zero words among a thread's 16
template <typename F>
__device__ __forceinline__ void ip_runs(const unsigned (&v)[IP_PPT], F f) {
  unsigned change = 1u, some = v[0] ? 1u : 0u;
#pragma unroll
  for (int k = 1; k < IP_PPT; ++k) {
    if (v[k] != v[k - 1]) change |= 1u << k;
    if (v[k]) some |= 1u << k;
  }
  unsigned starts = change & some;
  while (starts) {
    const int a = __builtin_ctz(starts);
    starts &= starts - 1u;
    const unsigned rest = change >> (a + 1);
    const int e = rest ? a + 1 + __builtin_ctz(rest) : IP_PPT;
    f(ip_pick(v, a), a, e - a);
  }
}

// the edge of pixel `me` towards neighbour `nb`: (me's ordinal, nb's class) where me has an ordinal, nb another one or none and a class
__device__ __forceinline__ unsigned ip_edge(unsigned me, unsigned nb, unsigned nc) {
  return (me >> 8) != 0u && (nb >> 8) != (me >> 8) && (nb & 255u) < nc ? (me & ~255u) | (nb & 255u) : 0u;
}

template <bool WIDE>
__global__ __launch_bounds__(IP_THREADS) void instance_parts_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ comps,
                                                                    unsigned long long* parts, unsigned long long* contacts, int H, int W,
                                                                    int nc, int K, int tiles_x, int tiles_per_frame) {
  __shared__ IpTable tb;
  __shared__ __attribute__((aligned(16))) unsigned tile[(IP_TH + 2) * IP_RS];      // rows 0 and IP_TH + 1: the halo above and below
  __shared__ unsigned side[2 * IP_TH];                                              // the halo left and right of the tile's rows
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < IP_SLOTS; i += IP_THREADS) {
    tb.key[i] = 0u;
    tb.touch[i] = 0u;
  }
  for (int i = tid; i < 6 * IP_SLOTS; i += IP_THREADS) tb.sums[i] = 0ull;
  for (int i = tid; i < 4 * IP_SLOTS; i += IP_THREADS) tb.ext[i] = 0u;
  const int f = (int)(blockIdx.x / (unsigned)tiles_per_frame);
  const int t = (int)(blockIdx.x % (unsigned)tiles_per_frame);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y0 = ty * IP_TH, xt = tx * IP_TW;
  const unsigned char* lf = labels + (long)f * H * W;
  const int* cf = comps + (long)f * H * W;
  const int r = tid / IP_CPR, ch = tid - r * IP_CPR;
  const int y = y0 + r, x0 = xt + ch * IP_PPT;
  unsigned w[IP_PPT];
#pragma unroll
  for (int k = 0; k < IP_PPT; ++k) w[k] = IP_NONE;
  if (y < H && x0 < W) {
    const long at = (long)y * W + x0;
    if (WIDE) {                                                // (W % 16 == 0: the 16 pixels exist)
      const uint4 lw = *reinterpret_cast<const uint4*>(lf + at);
      const int4* cp = reinterpret_cast<const int4*>(cf + at);
#pragma unroll
      for (int q = 0; q < IP_PPT / 4; ++q) {
        const int4 c = cp[q];
        w[4 * q] = ip_word(c.x, lm_byte(lw, 4 * q), K);
        w[4 * q + 1] = ip_word(c.y, lm_byte(lw, 4 * q + 1), K);
        w[4 * q + 2] = ip_word(c.z, lm_byte(lw, 4 * q + 2), K);
        w[4 * q + 3] = ip_word(c.w, lm_byte(lw, 4 * q + 3), K);
      }
    } else {
#pragma unroll
      for (int k = 0; k < IP_PPT; ++k)
        if (x0 + k < W) w[k] = ip_word(cf[at + k], (unsigned)lf[at + k], K);
    }
  }
  uint4* own = reinterpret_cast<uint4*>(tile + (r + 1) * IP_RS + ch * IP_PPT);
#pragma unroll
  for (int q = 0; q < IP_PPT / 4; ++q) own[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  for (int i = tid; i < 2 * IP_TW + 2 * IP_TH; i += IP_THREADS) {
    int hy, hx;
    unsigned* d;
    if (i < IP_TW) {
      hy = y0 - 1, hx = xt + i, d = tile + i;
    } else if (i < 2 * IP_TW) {
      hy = y0 + IP_TH, hx = xt + i - IP_TW, d = tile + (IP_TH + 1) * IP_RS + (i - IP_TW);
    } else if (i < 2 * IP_TW + IP_TH) {
      hy = y0 + i - 2 * IP_TW, hx = xt - 1, d = side + (i - 2 * IP_TW);
    } else {
      hy = y0 + i - 2 * IP_TW - IP_TH, hx = xt + IP_TW, d = side + IP_TH + (i - 2 * IP_TW - IP_TH);
    }
    unsigned v = IP_NONE;
    if (hy >= 0 && hy < H && hx >= 0 && hx < W) {
      const long at = (long)hy * W + hx;
      v = ip_word(cf[at], (unsigned)lf[at], K);
    }
    *d = v;
  }
  __syncthreads();
  unsigned long long* pf = parts + (long)f * K * nc * 10;
  unsigned long long* qf = contacts + (long)f * K * nc;
  bool any = false;
#pragma unroll
  for (int k = 0; k < IP_PPT; ++k) any |= (w[k] >> 8) != 0u;
  if (any) {                                                   // (a thread of the background, or past the map, has nothing to add)
    const unsigned ncu = (unsigned)nc;
    unsigned v[IP_PPT];
#pragma unroll
    for (int k = 0; k < IP_PPT; ++k) v[k] = (w[k] >> 8) != 0u && (w[k] & 255u) < ncu ? w[k] : 0u;
    IpTable* tp = &tb;                                         // (the closures hold values only: nothing of theirs lives in memory)
    ip_runs(v, [=](unsigned word, int a, int n) {
      ip_moments(*tp, pf, nc, word, lm_run((unsigned)(x0 + a), (unsigned)n, (unsigned)y, (unsigned)H, (unsigned)W));
    });
    const auto touch = [=](unsigned word, int, int n) { ip_touch(*tp, qf, nc, word, (unsigned)n); };
    const uint4* above = reinterpret_cast<const uint4*>(tile + r * IP_RS + ch * IP_PPT);
    const uint4* below = reinterpret_cast<const uint4*>(tile + (r + 2) * IP_RS + ch * IP_PPT);
#pragma unroll
    for (int q = 0; q < IP_PPT / 4; ++q) {
      const uint4 u = above[q];
      v[4 * q] = ip_edge(w[4 * q], u.x, ncu);
      v[4 * q + 1] = ip_edge(w[4 * q + 1], u.y, ncu);
      v[4 * q + 2] = ip_edge(w[4 * q + 2], u.z, ncu);
      v[4 * q + 3] = ip_edge(w[4 * q + 3], u.w, ncu);
    }
    ip_runs(v, touch);
#pragma unroll
    for (int q = 0; q < IP_PPT / 4; ++q) {
      const uint4 u = below[q];
      v[4 * q] = ip_edge(w[4 * q], u.x, ncu);
      v[4 * q + 1] = ip_edge(w[4 * q + 1], u.y, ncu);
      v[4 * q + 2] = ip_edge(w[4 * q + 2], u.z, ncu);
      v[4 * q + 3] = ip_edge(w[4 * q + 3], u.w, ncu);
    }
    ip_runs(v, touch);
    const unsigned lft = ch ? tile[(r + 1) * IP_RS + ch * IP_PPT - 1] : side[r];
    const unsigned rgt = ch < IP_CPR - 1 ? tile[(r + 1) * IP_RS + (ch + 1) * IP_PPT] : side[IP_TH + r];
#pragma unroll
    for (int k = 0; k < IP_PPT; ++k) v[k] = ip_edge(w[k], k ? w[k - 1] : lft, ncu);
    ip_runs(v, touch);
#pragma unroll
    for (int k = 0; k < IP_PPT; ++k) v[k] = ip_edge(w[k], k < IP_PPT - 1 ? w[k + 1] : rgt, ncu);
    ip_runs(v, touch);
  }
  __syncthreads();
  for (int i = tid; i < IP_SLOTS * 11; i += IP_THREADS) {
    const int s = i / 11, k = i - 11 * s;
    const unsigned word = tb.key[s];
    if (!word) continue;
    const long at = ip_at(word, nc);
    if (k < 6) {
      const unsigned long long sum = tb.sums[6 * s + k];
      if (sum) atomicAdd(pf + at * 10 + k, sum);
    } else if (k < 10) {
      const unsigned e = tb.ext[4 * s + k - 6];
      if (e) atomicMax(pf + at * 10 + k, (unsigned long long)e);
    } else if (tb.touch[s]) {
      atomicAdd(qf + at, (unsigned long long)tb.touch[s]);
    }
  }
}

extern "C" int stswin_instance_parts(const unsigned char* labels, const int* components, long long* parts, long long* contacts, int n,
                                     int H, int W, int nc, int K, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1890;
  if (labels == nullptr || components == nullptr || parts == nullptr || contacts == nullptr) return -1891;
  if (nc < 1 || nc > 64) return -1892;
  if (K < 1 || K > 1024) return -1893;
  if (((uintptr_t)components & 3) || (((uintptr_t)parts | (uintptr_t)contacts) & 7)) return -1894;
  const int tiles_x = (W + IP_TW - 1) / IP_TW;
  const long tpf = (long)tiles_x * ((H + IP_TH - 1) / IP_TH);
  if (tpf * n > 0x7fffffffL) return -1890;
  const bool wide = (((uintptr_t)labels | (uintptr_t)components) & 15) == 0 && W % IP_PPT == 0;
  dim3 grid((unsigned)(tpf * n));
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* p = reinterpret_cast<unsigned long long*>(parts);
  unsigned long long* q = reinterpret_cast<unsigned long long*>(contacts);
  stswin_zero_bytes(parts, (size_t)n * K * nc * 10 * sizeof(long long), st);        // (a kernel, not hipMemsetAsync: see common.h)
  stswin_zero_bytes(contacts, (size_t)n * K * nc * sizeof(long long), st);
  if (wide) hipLaunchKernelGGL(instance_parts_kernel<true>, grid, dim3(IP_THREADS), 0, st, labels, components, p, q, H, W, nc, K, tiles_x, (int)tpf);
  else hipLaunchKernelGGL(instance_parts_kernel<false>, grid, dim3(IP_THREADS), 0, st, labels, components, p, q, H, W, nc, K, tiles_x, (int)tpf);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_instance_parts_geometry(int which) {
  return which == 0 ? IP_TH : which == 1 ? IP_TW : which == 2 ? IP_SLOTS : -1;
}

// Connected components of a label map and their moments rows (stswincl_amd/utils/instruments.py, label_components, states the
// result; VideoSegmenter(instances=K)): block-based union-find on an int32 parent map of frame-local pixel indices y W + x.  A link
// only ever points to a smaller index of the same component (LDS or global atomicMin), so a component's root is its first pixel in
// raster order and every loop below is a root chase or a compare-and-lower that ends because a value strictly decreased: no kernel
// waits on another workgroup - no flag, ticket or look-back - and the launch boundaries are the only ordering between the passes.
//   1 cc_tile_kernel    a workgroup labels one CC_TH x CC_TW tile in LDS.  A tile row is one wave: a ballot of "differs from the left
//                       neighbour" gives every pixel the first pixel of its horizontal run; runs of neighbouring rows are joined
//                       (cc_union in LDS) once per stretch of pixels under the same upper run; then a root chase, and parent = the
//                       frame-local index of the pixel's in-tile root, -1 for a pixel of a skipped class or a class >= nc
//   2 cc_border_kernel  a thread per pixel of a tile's first row (first column) joins it with the pixel it faces across the border,
//                       or with a diagonal one (8-connectivity), once per stretch and pair of tiles: cc_union on the global map
//   3 cc_count_kernel   every pixel's parent becomes its root; a workgroup counts the roots of its raster chunk of CC_CHUNK pixels
//   4 cc_scan_kernel    one workgroup per frame: exclusive scan of the chunk counts (in place) and the frame's total
//   5 cc_number_kernel  a root's ordinal = its chunk's offset + its rank in the chunk (raster order, so truncation keeps the first K);
//                       the ordinal goes into `components` at the root, class and first pixel into its row
//   6 cc_rows_kernel    a thread takes up to CC_PPT pixels of one row: components = the root's ordinal for every other pixel, and
//                       the ten moments terms into rows[ordinal] for ordinals < K.  As label_moments_kernel does for labels: a full
//                       chunk of one component is pre-added across the wave per distinct ordinal (DPP sums of small numbers, lane
//                       63 expands them), a chunk with several runs adds run by run, both into the workgroup's LDS table of the
//                       instances it meets, which ends as one 64-bit global atomic per non-zero entry.
// Integer atomics only: exact and independent of the order.  rows is cleared by a fill kernel; every other word that is read was
// written by an earlier pass (parent, counts, total and components in full).  No kernel uses scratch memory.
#define CC_TH 16
#define CC_TW 64
#define CC_CHUNK 2048
#define CC_PPT 8
#define CC_THREADS 256

__device__ __forceinline__ bool cc_valid(unsigned l, int nc, unsigned long long skip) { return l < (unsigned)nc && !((skip >> (l & 63u)) & 1ull); }

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Join the sets of a and b; P[i] <= i always.  Each turn either ends or continues with a strictly smaller a.
template <typename Find>
__device__ __forceinline__ void cc_union(int* P, int a, int b, Find find) {
  for (;;) {
    a = find(P, a);
    b = find(P, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(P + a, b);          // a was a root when read: link it below b, unless someone lowered it first
    if (old == a) return;
    a = old;
  }
}

struct CcFindLds {
  __device__ __forceinline__ int operator()(const int* P, int a) const {
    int p;
    while ((p = ((const volatile int*)P)[a]) != a) a = p;
    return a;
  }
};
struct CcFindGlobal {
  __device__ __forceinline__ int operator()(const int* P, int a) const {
    int p;
    while ((p = cc_load(P + a)) != a) a = p;
    return a;
  }
};

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const unsigned char* __restrict__ labels, int* __restrict__ parent, int H, int W,
                                                             int nc, unsigned long long skip, int conn8, int tiles_x, int tiles_y) {
  __shared__ unsigned char cls[CC_TH * CC_TW];
  __shared__ int L[CC_TH * CC_TW];
  const int tile = (int)(blockIdx.x % (unsigned)(tiles_x * tiles_y)), f = (int)(blockIdx.x / (unsigned)(tiles_x * tiles_y));
  const int y0 = tile / tiles_x * CC_TH, x0 = tile % tiles_x * CC_TW;
  const unsigned char* lab = labels + (long)f * H * W;
  int* par = parent + (long)f * H * W;
  const int tx = (int)threadIdx.x & (CC_TW - 1), ty0 = (int)threadIdx.x / CC_TW;      // rows ty0, ty0 + 4, ty0 + 8, ty0 + 12
  bool start[4];                                                                        // (constant indices only: registers)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ty = ty0 + 4 * j, i = ty * CC_TW + tx, y = y0 + ty, x = x0 + tx;
    unsigned l = 255u;                                                                  // 255: not part of any component
    if (y < H && x < W) {
      l = lab[(long)y * W + x];
      if (!cc_valid(l, nc, skip)) l = 255u;
    }
    cls[i] = (unsigned char)l;
    // a tile row is one wave: every pixel starts at the first pixel of its horizontal run (the highest start bit at or below tx)
    const unsigned left = (unsigned)__shfl_up((int)l, 1);
    start[j] = tx == 0 || left != l;
    const unsigned long long below = __ballot(start[j]) & (~0ull >> (63 - tx));
    L[i] = ty * CC_TW + 63 - __clzll((long long)below);
  }
  __syncthreads();
  // join the runs of neighbouring rows, once per stretch of pixels that lie under the same upper run: where the stretch begins.  A
  // diagonal neighbour only matters where the upper neighbour is of another class (else it belongs to the upper neighbour's run),
  // the upper left one only at the start of a run (else the pixel to the left lies under that run)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ty = ty0 + 4 * j, i = ty * CC_TW + tx;
    const unsigned l = cls[i];
    if (l == 255u || ty == 0) continue;
    if (cls[i - CC_TW] == l) {
      if (start[j] || cls[i - CC_TW - 1] != l) cc_union(L, i, i - CC_TW, CcFindLds());
    } else if (conn8) {
      if (start[j] && tx > 0 && cls[i - CC_TW - 1] == l) cc_union(L, i, i - CC_TW - 1, CcFindLds());
      if (tx < CC_TW - 1 && cls[i - CC_TW + 1] == l) cc_union(L, i, i - CC_TW + 1, CcFindLds());
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ty = ty0 + 4 * j, i = ty * CC_TW + tx, y = y0 + ty, x = x0 + tx;
    if (y < H && x < W) {
      int r = -1;
      if (cls[i] != 255u) {
        const int t = CcFindLds()(L, i);
        r = (y0 + t / CC_TW) * W + x0 + t % CC_TW;
      }
      par[(long)y * W + x] = r;
    }
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_border_kernel(const unsigned char* __restrict__ labels, int* parent, int H, int W, int nc,
                                                               unsigned long long skip, int conn8, long rows_items, long per_frame, long items) {
  const long g = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (g >= items) return;                  // (the grid's tail)
  const int f = (int)(g / per_frame);
  long q = g - (long)f * per_frame;
  const unsigned char* lab = labels + (long)f * H * W;
  int* par = parent + (long)f * H * W;
  // the pixel (y, x), the step (dy, dx) across the border and the step (ay, ax) along it, t its position along the border of length n,
  // edge the length of one tile's side along it
  int y, x, dy, dx, ay, ax, t, n, edge;
  if (q < rows_items) {
    y = (int)(q / W + 1) * CC_TH;
    x = (int)(q % W);
    dy = -1, dx = 0, ay = 0, ax = 1, t = x, n = W, edge = CC_TW;
  } else {
    q -= rows_items;
    x = (int)(q / H + 1) * CC_TW;
    y = (int)(q % H);
    dy = 0, dx = -1, ay = 1, ax = 0, t = y, n = H, edge = CC_TH;
  }
  const unsigned l = lab[(long)y * W + x];
  if (!cc_valid(l, nc, skip)) return;
  const int p = y * W + x, across = (y + dy) * W + x + dx, along = ay * W + ax;
  // as in the tile: one union per stretch of border pixels that face the same run on the other side, where the stretch begins - and
  // where the next pair of tiles begins, whose pixels nothing has joined with the last pair's yet; a diagonal neighbour only where
  // the facing pixel is of another class, the backward one only at the start of this side's run (else the pixel before faces it)
  const bool first = t == 0 || lab[p - along] != l;
  if (lab[across] == l) {
    if (first || t % edge == 0 || lab[across - along] != l) cc_union(par, p, across, CcFindGlobal());
  } else if (conn8) {
    if (first && t > 0 && lab[across - along] == l) cc_union(par, p, across - along, CcFindGlobal());
    if (t < n - 1 && lab[across + along] == l) cc_union(par, p, across + along, CcFindGlobal());
  }
}

// the workgroup's sum of v in every thread (CC_THREADS = 4 waves); `red` is 4 words of LDS
__device__ __forceinline__ unsigned cc_block_sum(unsigned v, unsigned* red) {
  const unsigned w = lm_wave<false>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = w;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(int* parent, int* __restrict__ counts, int HW, int chunks) {
  __shared__ unsigned red[4];
  const int ch = (int)(blockIdx.x % (unsigned)chunks), f = (int)(blockIdx.x / (unsigned)chunks);
  int* par = parent + (long)f * HW;
  const int base = ch * CC_CHUNK + (int)threadIdx.x * CC_PPT;
  unsigned c = 0;
#pragma unroll
  for (int i = 0; i < CC_PPT; ++i) {
    const int p = base + i;
    if (p < HW) {
      int a = par[p];
      if (a >= 0) {
        if (a != p) {
          a = CcFindGlobal()(par, a);
          par[p] = a;                        // (a reader sees the old link or the root: both lead to the root)
        } else {
          c += 1u;
        }
      }
    }
  }
  c = cc_block_sum(c, red);
  if (threadIdx.x == 0) counts[(long)f * chunks + ch] = (int)c;
}

// inclusive scan of v over the workgroup's threads; `red` is 4 words of LDS
__device__ __forceinline__ unsigned cc_block_scan(unsigned v, unsigned* red) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o);
    if ((int)(threadIdx.x & 63) >= o) v += t;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int w = threadIdx.x >> 6;
  return v + (w > 0 ? red[0] : 0u) + (w > 1 ? red[1] : 0u) + (w > 2 ? red[2] : 0u);
}

__global__ __launch_bounds__(CC_THREADS) void cc_scan_kernel(int* counts, int* __restrict__ total, int chunks) {
  __shared__ unsigned red[4];
  int* c = counts + (long)blockIdx.x * chunks;
  unsigned carry = 0;
  for (int base = 0; base < chunks; base += CC_THREADS) {
    const int i = base + (int)threadIdx.x;
    const unsigned v = i < chunks ? (unsigned)c[i] : 0u;
    const unsigned incl = cc_block_scan(v, red);
    if (i < chunks) c[i] = (int)(carry + incl - v);
    carry += red[0] + red[1] + red[2] + red[3];
  }
  if (threadIdx.x == 0) total[blockIdx.x] = (int)carry;
}

__global__ __launch_bounds__(CC_THREADS) void cc_number_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ parent,
                                                               const int* __restrict__ offsets, int* __restrict__ comp,
                                                               unsigned long long* __restrict__ rows, int HW, int chunks, int K) {
  __shared__ unsigned red[4];
  const int ch = (int)(blockIdx.x % (unsigned)chunks), f = (int)(blockIdx.x / (unsigned)chunks);
  const int* par = parent + (long)f * HW;
  const int base = ch * CC_CHUNK + (int)threadIdx.x * CC_PPT;
  unsigned mask = 0;                         // bit i: pixel base + i is a root
#pragma unroll
  for (int i = 0; i < CC_PPT; ++i)
    if (base + i < HW && par[base + i] == base + i) mask |= 1u << i;
  const unsigned mine = (unsigned)__builtin_popcount(mask);
  unsigned o = (unsigned)offsets[(long)f * chunks + ch] + cc_block_scan(mine, red) - mine;
#pragma unroll
  for (int i = 0; i < CC_PPT; ++i)
    if (mask & (1u << i)) {
      const int p = base + i;
      comp[(long)f * HW + p] = (int)o;
      if (o < (unsigned)K) {
        unsigned long long* r = rows + ((long)f * K + o) * 12;
        r[0] = labels[(long)f * HW + p];
        r[1] = (unsigned long long)p;
      }
      ++o;
    }
}

__device__ __forceinline__ void cc_flush(unsigned long long* r, const LmTerms& t) {      // r: the instance's row
  atomicAdd(r + 2, (unsigned long long)t.n);
  atomicAdd(r + 3, (unsigned long long)t.sx);
  atomicAdd(r + 4, (unsigned long long)t.sy);
  atomicAdd(r + 5, t.sxx);
  atomicAdd(r + 6, t.sxy);
  atomicAdd(r + 7, t.syy);
  atomicMax(r + 8, (unsigned long long)t.e0);
  atomicMax(r + 9, (unsigned long long)t.e1);
  atomicMax(r + 10, (unsigned long long)t.e2);
  atomicMax(r + 11, (unsigned long long)t.e3);
}

// The workgroup's table of the instances it meets: slot ord % CC_SLOTS belongs to the first ordinal that claims it (compare-and-swap
// on its tag), later ordinals of the same slot go to the global row directly.  Nothing waits: a claim succeeds or the other path is taken.
#define CC_SLOTS 32

struct CcTable {
  int tag[CC_SLOTS];
  unsigned long long sums[CC_SLOTS * 6];
  unsigned ext[CC_SLOTS * 4];
};

__device__ __forceinline__ void cc_add(CcTable& tb, unsigned long long* frows, int ord, const LmTerms& t) {
  const int slot = ord & (CC_SLOTS - 1);
  int owner = ((volatile int*)tb.tag)[slot];
  if (owner == -1) {
    owner = atomicCAS(&tb.tag[slot], -1, ord);
    if (owner == -1) owner = ord;
  }
  if (owner == ord) lm_flush(tb.sums, tb.ext, (unsigned)slot, t);
  else cc_flush(frows + (long)ord * 12, t);
}

__global__ __launch_bounds__(CC_THREADS) void cc_rows_kernel(const int* __restrict__ parent, int* comp, unsigned long long* rows, int H, int W,
                                                             int K, int cpr, int blocks_per_frame) {
  __shared__ CcTable tb;
  for (int i = threadIdx.x; i < CC_SLOTS; i += CC_THREADS) tb.tag[i] = -1;
  for (int i = threadIdx.x; i < CC_SLOTS * 6; i += CC_THREADS) tb.sums[i] = 0ull;
  for (int i = threadIdx.x; i < CC_SLOTS * 4; i += CC_THREADS) tb.ext[i] = 0u;
  __syncthreads();
  const int f = (int)(blockIdx.x / (unsigned)blocks_per_frame);
  const int q = (int)(blockIdx.x % (unsigned)blocks_per_frame) * CC_THREADS + (int)threadIdx.x;
  const int row = q / cpr, col = q - row * cpr;
  const bool valid = row < H;                                  // (the wave's lanes with a chunk are a prefix)
  const int len = valid ? min(CC_PPT, W - CC_PPT * col) : 0;
  const long fo = (long)f * H * W;
  const int p0 = row * W + CC_PPT * col;
  const int* par = parent + fo;
  int* cmp = comp + fo;
  unsigned long long* frows = rows + (long)f * K * 12;
  // runs of one root, left to right; the chunk is `full` when it is one run of CC_PPT pixels of a component
  int run_root = -2, run_start = 0, run_ord = -1, ord = -1;      // ord: a full chunk's ordinal
  bool full = false;
#pragma unroll
  for (int i = 0; i <= CC_PPT; ++i) {
    const int r = i < len ? par[p0 + i] : -2;
    if (r != run_root) {
      if (run_root >= 0) {                                     // the run [run_start, i) ends here
        if (run_start == 0 && i == CC_PPT) full = true, ord = run_ord;
        else if (run_ord < K)
          cc_add(tb, frows, run_ord, lm_run((unsigned)(CC_PPT * col + run_start), (unsigned)(i - run_start), (unsigned)row, (unsigned)H, (unsigned)W));
      }
      run_root = r;
      run_start = i;
      run_ord = r >= 0 ? cmp[r] : -1;                          // (written at the roots by cc_number_kernel; this kernel writes the others)
    }
    if (i < len && r != p0 + i) cmp[p0 + i] = run_ord;
  }
  // the full chunks, ordinal by ordinal (wave-uniform from here: every lane takes part in the sums)
  const unsigned row_w = (unsigned)__builtin_amdgcn_readfirstlane(row);       // lane 0's row: the smallest of the wave
  const unsigned cx = (unsigned)col, dy = (unsigned)row - row_w;              // cx < 2048, dy <= 64 / cpr + 1
  unsigned long long todo = __ballot(full && ord < K);
  while (todo) {
    const int first = __ffsll((long long)todo) - 1;
    const int O = __builtin_amdgcn_readlane(ord, first);
    const bool mine = full && ord == O;
    const unsigned long long m = __ballot(mine);
    todo &= ~m;
    const int last = 63 - __clzll((long long)m);
    const unsigned mcx = mine ? cx : 0u, mdy = mine ? dy : 0u;
    // <= 64 lanes of cx < 2048, dy <= 65: every sum stays below 2^32; the count and sum dy share a word (64 < 2^8)
    const unsigned c_sdy = lm_wave<false>((mine ? 1u : 0u) | (mdy << 8));
    const unsigned scx = lm_wave<false>(mcx), scx2 = lm_wave<false>(mcx * mcx), scxdy = lm_wave<false>(mcx * mdy);
    const unsigned sdy2 = lm_wave<false>(mdy * mdy);
    const unsigned cx_max = lm_wave<true>(mcx), cx_min = 2047u - lm_wave<true>(mine ? 2047u - cx : 0u);
    const unsigned dy_min = (unsigned)__builtin_amdgcn_readlane((int)dy, first), dy_max = (unsigned)__builtin_amdgcn_readlane((int)dy, last);
    if ((threadIdx.x & 63) == 63) {
      const unsigned c = c_sdy & 255u, sdy = c_sdy >> 8;
      const unsigned sy = c * row_w + sdy;                                                      // sum of the chunks' rows
      const unsigned long long scxy = (unsigned long long)row_w * scx + scxdy;
      const unsigned long long sy2 = (unsigned long long)c * (row_w * row_w) + (unsigned long long)(2u * row_w * sdy + sdy2);
      LmTerms t;                       // sum_{i<8} (8 cx + i) = 64 cx + 28, sum (8 cx + i)^2 = 512 cx^2 + 448 cx + 140
      t.n = 8u * c;
      t.sx = 64u * scx + 28u * c;
      t.sy = 8u * sy;
      t.sxx = 512ull * scx2 + (unsigned long long)(448u * scx + 140u * c);
      t.sxy = 64ull * scxy + 28ull * sy;
      t.syy = 8ull * sy2;
      t.e0 = (unsigned)W - 8u * cx_min;
      t.e1 = (unsigned)H - (row_w + dy_min);
      t.e2 = 8u * cx_max + 8u;
      t.e3 = row_w + dy_max + 1u;
      cc_add(tb, frows, O, t);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CC_SLOTS * 10; i += CC_THREADS) {        // the table's non-zero entries into the rows of their owners
    const int slot = i / 10, k = i - 10 * slot, owner = tb.tag[slot];
    if (owner < 0) continue;
    unsigned long long* o = frows + (long)owner * 12 + 2 + k;
    if (k < 6) {
      const unsigned long long v = tb.sums[6 * slot + k];
      if (v) atomicAdd(o, v);
    } else {
      const unsigned e = tb.ext[4 * slot + k - 6];
      if (e) atomicMax(o, (unsigned long long)e);
    }
  }
}

extern "C" int stswin_label_components_geometry(int which) { return which == 0 ? CC_TH : which == 1 ? CC_TW : which == 2 ? CC_CHUNK : -1; }

extern "C" long stswin_label_components_scratch(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1830;
  const long HW = (long)H * W, chunks = (HW + CC_CHUNK - 1) / CC_CHUNK;
  return 4 * (long)n * (HW + chunks);                    // the parent map, then the chunk counts
}

extern "C" int stswin_label_components(const unsigned char* labels, int* components, long long* rows, int* total, int n, int H, int W, int nc,
                                       int connectivity, long skip, int K, void* workspace, long workspace_bytes, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1830;
  if (labels == nullptr || components == nullptr || rows == nullptr || total == nullptr || workspace == nullptr) return -1831;
  if (nc < 1 || nc > 64) return -1832;
  if (connectivity != 4 && connectivity != 8) return -1833;
  if (K < 1 || K > 1024) return -1834;
  if (workspace_bytes < stswin_label_components_scratch(n, H, W) || ((uintptr_t)workspace & 3)) return -1835;
  const int HW = H * W, chunks = (HW + CC_CHUNK - 1) / CC_CHUNK;
  const int tiles_x = (W + CC_TW - 1) / CC_TW, tiles_y = (H + CC_TH - 1) / CC_TH;
  const int cpr = (W + CC_PPT - 1) / CC_PPT;
  const long bpf = ((long)H * cpr + CC_THREADS - 1) / CC_THREADS;
  const long rows_items = (long)(tiles_y - 1) * W, per_frame = rows_items + (long)(tiles_x - 1) * H;
  const long border_blocks = (per_frame * n + CC_THREADS - 1) / CC_THREADS;
  if ((long)tiles_x * tiles_y * n > 0x7fffffffL || (long)chunks * n > 0x7fffffffL || bpf * n > 0x7fffffffL || border_blocks > 0x7fffffffL)
    return -1830;
  hipStream_t st = (hipStream_t)stream;
  int* parent = reinterpret_cast<int*>(workspace);
  int* counts = parent + (long)n * HW;
  unsigned long long* r = reinterpret_cast<unsigned long long*>(rows);
  const unsigned long long sk = (unsigned long long)skip;
  const int conn8 = connectivity == 8;
  stswin_zero_bytes(rows, sizeof(long long) * 12 * (size_t)K * (size_t)n, st);         // (a kernel, not hipMemsetAsync: see common.h)
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(tiles_x * tiles_y * n)), dim3(CC_THREADS), 0, st, labels, parent, H, W, nc, sk, conn8, tiles_x,
                     tiles_y);
  if (per_frame > 0)
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)border_blocks), dim3(CC_THREADS), 0, st, labels, parent, H, W, nc, sk, conn8, rows_items,
                       per_frame, per_frame * n);
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)(chunks * n)), dim3(CC_THREADS), 0, st, parent, counts, HW, chunks);
  hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)n), dim3(CC_THREADS), 0, st, counts, total, chunks);
  hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)(chunks * n)), dim3(CC_THREADS), 0, st, labels, (const int*)parent, (const int*)counts,
                     components, r, HW, chunks, K);
  hipLaunchKernelGGL(cc_rows_kernel, dim3((unsigned)(bpf * n)), dim3(CC_THREADS), 0, st, (const int*)parent, components, r, H, W, K, cpr, (int)bpf);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// The label map cleaned: specks out, holes filled (stswincl_amd/utils/instruments.py, clean_labels, states the result;
// VideoSegmenter(clean_area=A)).  The components are those of the union-find above with nothing skipped; a component of fewer than
// min_area pixels whose class is not kept is small, and takes the class most of its pixel edges towards stable pixels lead to.  The
// workspace, in int32 words: the parent map [n][H W], aux [n][H W] (at a root: first the component's area, then -1 for a stable
// component and the ordinal s among the frame's small ones otherwise), the chunk counts, the frames' totals [n], info [n][max_small][2]
// (root, then area, then the new label) and votes [n][max_small][nc].  Launches:
//   1, 2 fill kernels          aux and votes to zero
//   3, 4 cc_tile_kernel, cc_border_kernel (the latter only with more than one tile), 5 cc_count_kernel: every pixel's parent is its root
//   6 cl_area_kernel           a thread folds the runs of equal roots along its CL_PPT pixels of a row and adds each run to the keyed LDS
//                              table of its tile (as launch 10 does), which ends as one global atomic per root the tile meets
//   7 cl_count_kernel          a workgroup counts the small roots of its raster chunk of CC_CHUNK pixels;  8 cc_scan_kernel as above
//   9 cl_number_kernel         a small root's s = its chunk's offset + its rank in the chunk (raster order: truncation keeps the first
//                              max_small); aux = s and info = (root, area) for s < max_small, aux = -1 at a stable root; stats
//  10 cl_vote_kernel           a workgroup takes a tile of CL_TH x CL_TW pixels; only the pixels of small components with s < max_small
//                              do any work: each looks at its four neighbours' roots and adds a vote for a stable one's class to the
//                              workgroup's keyed LDS table (CL_SLOTS slots, multiplicative hash, CL_PROBES probes), whose slots in use
//                              end as one global atomic each; a key that finds no slot adds to votes directly, with the same result
//  11 cl_resolve_kernel        a thread per small component: the first maximum; the area into stats where the label changes
//  12 cl_relabel_kernel        out = the new label for the pixels of small components with s < max_small, the label elsewhere
// Integer atomics only: exact and independent of the order.  No kernel waits on another workgroup or uses scratch memory.  WIDE:
// labels, out and the workspace 16-byte aligned and W % 16 == 0, 16-byte loads and stores; else element by element.
#define CL_TH 32
#define CL_TW 128
#define CL_PPT 16
#define CL_CPR (CL_TW / CL_PPT)
#define CL_THREADS (CL_TH * CL_CPR)
#define CL_SLOTS 256
#define CL_PROBES 8
static_assert(CL_SLOTS == 256, "cl_vote takes the hash's top 8 bits");

// the thread's pixels: row y, columns x0 .. x0 + len - 1 of frame f (len 0: none)
struct ClSpan {
  int f, y, x0, len;
};

__device__ __forceinline__ ClSpan cl_span(int H, int W, int tiles_x, int tiles_per_frame) {
  ClSpan s;
  s.f = (int)(blockIdx.x / (unsigned)tiles_per_frame);
  const int t = (int)(blockIdx.x % (unsigned)tiles_per_frame);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int r = (int)threadIdx.x / CL_CPR, ch = (int)threadIdx.x - r * CL_CPR;
  s.y = ty * CL_TH + r;
  s.x0 = tx * CL_TW + ch * CL_PPT;
  s.len = s.y < H ? max(0, min(CL_PPT, W - s.x0)) : 0;
  return s;
}

template <bool WIDE>
__device__ __forceinline__ void cl_roots(const int* __restrict__ par, int len, int (&r)[CL_PPT]) {      // -1 past the end
  if (WIDE) {
    const int4* p = reinterpret_cast<const int4*>(par);
#pragma unroll
    for (int q = 0; q < CL_PPT / 4; ++q) {
      const int4 v = p[q];
      r[4 * q] = v.x;
      r[4 * q + 1] = v.y;
      r[4 * q + 2] = v.z;
      r[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CL_PPT; ++k) r[k] = k < len ? par[k] : -1;
  }
}

// The workgroup's keyed table of CL_SLOTS counters in LDS: `word` (non-zero) finds its slot by a multiplicative hash and up to CL_PROBES
// linear probes, claiming a free one by compare-and-swap, and adds v there -> true; false when none of its probe slots is free or its
// own (always so once the table is full): the caller then adds to global memory directly, the same integers either way.
__device__ __forceinline__ bool cl_table_add(unsigned* key, unsigned* cnt, unsigned word, unsigned v) {
  const unsigned h = (word * 2654435761u) >> 24;
  for (int t = 0; t < CL_PROBES; ++t) {
    const unsigned i = (h + t) & (CL_SLOTS - 1);
    const unsigned old = atomicCAS(&key[i], 0u, word);
    if (old == 0u || old == word) {
      atomicAdd(&cnt[i], v);
      return true;
    }
  }
  return false;
}

// (a large component - the background - covers whole tiles: its runs meet in one LDS counter and leave as one global atomic per tile;
// added run by run to the one word at its root they would queue up behind each other across the whole device)
template <bool WIDE>
__global__ __launch_bounds__(CL_THREADS) void cl_area_kernel(const int* __restrict__ parent, int* aux, int H, int W, int tiles_x,
                                                             int tiles_per_frame) {
  __shared__ unsigned key[CL_SLOTS], cnt[CL_SLOTS];
  for (int i = threadIdx.x; i < CL_SLOTS; i += CL_THREADS) {
    key[i] = 0u;
    cnt[i] = 0u;
  }
  __syncthreads();
  const ClSpan s = cl_span(H, W, tiles_x, tiles_per_frame);
  int* ax = aux + (long)s.f * H * W;
  if (s.len > 0) {
    int r[CL_PPT];
    cl_roots<WIDE>(parent + (long)s.f * H * W + (long)s.y * W + s.x0, s.len, r);
    int cur = -1;
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k <= CL_PPT; ++k) {
      const int rk = k < CL_PPT ? r[k < CL_PPT ? k : 0] : -1;
      if (rk != cur) {
        if (cur >= 0 && !cl_table_add(key, cnt, (unsigned)cur + 1u, c)) atomicAdd(ax + cur, (int)c);
        cur = rk;
        c = 0;
      }
      c += 1;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CL_SLOTS; i += CL_THREADS)
    if (key[i]) atomicAdd(ax + (key[i] - 1u), (int)cnt[i]);
}

// bit i: pixel base + i is the root of a small component (aux still holds the areas)
__device__ __forceinline__ unsigned cl_small_roots(const unsigned char* __restrict__ lab, const int* __restrict__ par,
                                                   const int* __restrict__ aux, int base, int HW, int min_area, unsigned long long keep,
                                                   unsigned* roots) {
  unsigned small = 0, all = 0;
#pragma unroll
  for (int i = 0; i < CC_PPT; ++i) {
    const int p = base + i;
    if (p < HW && par[p] == p) {
      all |= 1u << i;
      if (aux[p] < min_area && !((keep >> (lab[p] & 63u)) & 1ull)) small |= 1u << i;
    }
  }
  *roots = all;
  return small;
}

__global__ __launch_bounds__(CC_THREADS) void cl_count_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ parent,
                                                              const int* __restrict__ aux, int* __restrict__ counts, int HW, int chunks,
                                                              int min_area, unsigned long long keep) {
  __shared__ unsigned red[4];
  const int ch = (int)(blockIdx.x % (unsigned)chunks), f = (int)(blockIdx.x / (unsigned)chunks);
  const long fo = (long)f * HW;
  unsigned roots;
  const unsigned small = cl_small_roots(labels + fo, parent + fo, aux + fo, ch * CC_CHUNK + (int)threadIdx.x * CC_PPT, HW, min_area, keep, &roots);
  const unsigned c = cc_block_sum((unsigned)__builtin_popcount(small), red);
  if (threadIdx.x == 0) counts[(long)f * chunks + ch] = (int)c;
}

__global__ __launch_bounds__(CC_THREADS) void cl_number_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ parent,
                                                               int* aux, const int* __restrict__ offsets, const int* __restrict__ total,
                                                               int* __restrict__ info, int* __restrict__ stats, int HW, int chunks,
                                                               int min_area, unsigned long long keep, int max_small) {
  __shared__ unsigned red[4];
  const int ch = (int)(blockIdx.x % (unsigned)chunks), f = (int)(blockIdx.x / (unsigned)chunks);
  const long fo = (long)f * HW;
  const int base = ch * CC_CHUNK + (int)threadIdx.x * CC_PPT;
  unsigned roots;
  const unsigned small = cl_small_roots(labels + fo, parent + fo, aux + fo, base, HW, min_area, keep, &roots);
  const unsigned mine = (unsigned)__builtin_popcount(small);
  unsigned o = (unsigned)offsets[(long)f * chunks + ch] + cc_block_scan(mine, red) - mine;
#pragma unroll
  for (int i = 0; i < CC_PPT; ++i) {
    if (!(roots & (1u << i))) continue;
    int* a = aux + fo + base + i;
    if (small & (1u << i)) {
      if (o < (unsigned)max_small) {
        int* e = info + ((long)f * max_small + o) * 2;
        e[0] = base + i;
        e[1] = *a;
      }
      *a = (int)o;
      ++o;
    } else {
      *a = -1;
    }
  }
  if (ch == 0 && threadIdx.x == 0) {
    stats[2 * f] = total[f];
    stats[2 * f + 1] = 0;
  }
}

__device__ __forceinline__ void cl_vote(unsigned* key, unsigned* cnt, int* votes_f, int nc, int s, unsigned c) {
  const unsigned word = ((unsigned)s << 6 | c) + 1u;                  // s < 65536, c < 64; 0: a free slot
  if (!cl_table_add(key, cnt, word, 1u)) atomicAdd(votes_f + (long)s * nc + c, 1);
}

template <bool WIDE>
__global__ __launch_bounds__(CL_THREADS) void cl_vote_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ parent,
                                                             const int* __restrict__ aux, int* votes, int H, int W, int nc, int max_small,
                                                             int tiles_x, int tiles_per_frame) {
  __shared__ unsigned key[CL_SLOTS], cnt[CL_SLOTS];
  for (int i = threadIdx.x; i < CL_SLOTS; i += CL_THREADS) {
    key[i] = 0u;
    cnt[i] = 0u;
  }
  __syncthreads();
  const ClSpan s = cl_span(H, W, tiles_x, tiles_per_frame);
  const long fo = (long)s.f * H * W;
  const unsigned char* lab = labels + fo;
  const int* par = parent + fo;
  const int* ax = aux + fo;
  int* votes_f = votes + (long)s.f * max_small * nc;
  if (s.len > 0) {
    const int p0 = s.y * W + s.x0;
    int r[CL_PPT];
    cl_roots<WIDE>(par + p0, s.len, r);
    unsigned todo = 0;                                   // the thread's pixels of small components with s < max_small
    int cur = -1;
    bool live = false;
#pragma unroll
    for (int k = 0; k < CL_PPT; ++k) {
      if (r[k] != cur) {
        cur = r[k];
        live = cur >= 0 && (unsigned)ax[cur] < (unsigned)max_small;
      }
      if (live) todo |= 1u << k;
    }
    while (todo) {                                       // (rare: the roots are read again rather than indexed out of registers)
      const int k = __builtin_ctz(todo);
      todo &= todo - 1u;
      const int x = s.x0 + k, p = p0 + k;
      const int sm = ax[par[p]];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int qy = s.y + (d == 0 ? -1 : d == 1 ? 1 : 0), qx = x + (d == 2 ? -1 : d == 3 ? 1 : 0);
        if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
        const int q = qy * W + qx, rq = par[q];
        if (rq >= 0 && ax[rq] == -1) cl_vote(key, cnt, votes_f, nc, sm, (unsigned)lab[q]);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < CL_SLOTS; i += CL_THREADS) {
    const unsigned word = key[i];
    if (word) atomicAdd(votes_f + (long)((word - 1u) >> 6) * nc + ((word - 1u) & 63u), (int)cnt[i]);
  }
}

__global__ __launch_bounds__(CC_THREADS) void cl_resolve_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ votes,
                                                                int* info, int* stats, int HW, int nc, int max_small,
                                                                int blocks_per_frame) {
  const int f = (int)(blockIdx.x / (unsigned)blocks_per_frame);
  const int s = (int)(blockIdx.x % (unsigned)blocks_per_frame) * CC_THREADS + (int)threadIdx.x;
  if (s >= max_small || s >= stats[2 * f]) return;       // (stats[2 f]: written by cl_number_kernel, only read here)
  int* e = info + ((long)f * max_small + s) * 2;
  const int old = (int)labels[(long)f * HW + e[0]], area = e[1];
  const int* v = votes + ((long)f * max_small + s) * nc;
  int best = 0, arg = old;
  for (int c = 0; c < nc; ++c) {
    const int t = v[c];
    if (t > best) best = t, arg = c;
  }
  e[1] = arg;
  if (arg != old) atomicAdd(stats + 2 * f + 1, area);
}

template <bool WIDE>
__global__ __launch_bounds__(CL_THREADS) void cl_relabel_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ parent,
                                                                const int* __restrict__ aux, const int* __restrict__ info,
                                                                unsigned char* __restrict__ out, int H, int W, int max_small, int tiles_x,
                                                                int tiles_per_frame) {
  const ClSpan s = cl_span(H, W, tiles_x, tiles_per_frame);
  if (s.len == 0) return;
  const long fo = (long)s.f * H * W, at = fo + (long)s.y * W + s.x0;
  const int* ax = aux + fo;
  const int* inf = info + (long)s.f * max_small * 2;
  int r[CL_PPT];
  cl_roots<WIDE>(parent + at, s.len, r);
  uint4 lw = make_uint4(0u, 0u, 0u, 0u);
  if (WIDE) lw = *reinterpret_cast<const uint4*>(labels + at);
  unsigned o[CL_PPT / 4] = {0u, 0u, 0u, 0u};
  int cur = -1, repl = -1;                               // repl: the new label of the run's component, -1: the pixel keeps its own
#pragma unroll
  for (int k = 0; k < CL_PPT; ++k) {
    if (r[k] != cur) {
      cur = r[k];
      repl = -1;
      if (cur >= 0) {
        const int sm = ax[cur];
        if ((unsigned)sm < (unsigned)max_small) repl = inf[2 * sm + 1];
      }
    }
    if (WIDE) {
      const unsigned v = repl >= 0 ? (unsigned)repl : lm_byte(lw, k);
      o[k >> 2] |= v << (8 * (k & 3));
    } else if (k < s.len) {
      out[at + k] = repl >= 0 ? (unsigned char)repl : labels[at + k];
    }
  }
  if (WIDE) *reinterpret_cast<uint4*>(out + at) = make_uint4(o[0], o[1], o[2], o[3]);
}

extern "C" int stswin_labels_clean_geometry(int which) {
  return which == 0 ? CL_TH : which == 1 ? CL_TW : which == 2 ? CC_CHUNK : which == 3 ? CL_SLOTS : -1;
}

struct ClLayout {
  long parent, aux, counts, total, info, votes, words;   // offsets in int32 words
  int chunks, tiles_x;
  long tpf, cc_tiles, border_items, resolve_bpf;
};

static bool cl_layout(int n, int H, int W, int nc, int max_small, ClLayout* L) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return false;
  const long HW = (long)H * W;
  L->chunks = (int)((HW + CC_CHUNK - 1) / CC_CHUNK);
  L->tiles_x = (W + CL_TW - 1) / CL_TW;
  L->tpf = (long)L->tiles_x * ((H + CL_TH - 1) / CL_TH);
  L->cc_tiles = (long)((W + CC_TW - 1) / CC_TW) * ((H + CC_TH - 1) / CC_TH);
  L->border_items = (long)((H + CC_TH - 1) / CC_TH - 1) * W + (long)((W + CC_TW - 1) / CC_TW - 1) * H;
  L->resolve_bpf = ((long)max_small + CC_THREADS - 1) / CC_THREADS;
  if (L->tpf * n > 0x7fffffffL || L->cc_tiles * n > 0x7fffffffL || (long)L->chunks * n > 0x7fffffffL ||
      (L->border_items * n + CC_THREADS - 1) / CC_THREADS > 0x7fffffffL || L->resolve_bpf * n > 0x7fffffffL)
    return false;
  L->parent = 0;
  L->aux = (long)n * HW;
  L->counts = 2 * (long)n * HW;
  L->total = L->counts + (long)n * L->chunks;
  L->info = L->total + n;
  L->votes = L->info + 2 * (long)n * max_small;
  L->words = L->votes + (long)n * max_small * nc;
  return true;
}

extern "C" long stswin_labels_clean_scratch(int n, int H, int W, int nc, int max_small) {
  ClLayout L;
  if (nc < 1 || nc > 64) return -1902;
  if (max_small < 1 || max_small > 65536) return -1905;
  if (!cl_layout(n, H, W, nc, max_small, &L)) return -1900;
  return 4 * L.words;
}

extern "C" int stswin_labels_clean(const unsigned char* labels, unsigned char* out, int* stats, int n, int H, int W, int nc, int connectivity,
                                   long keep, int min_area, int max_small, void* workspace, long workspace_bytes, void* stream) {
  ClLayout L;
  if (!cl_layout(n, H, W, nc < 1 || nc > 64 ? 1 : nc, max_small < 1 || max_small > 65536 ? 1 : max_small, &L)) return -1900;
  if (labels == nullptr || out == nullptr || stats == nullptr || workspace == nullptr) return -1901;
  if (nc < 1 || nc > 64) return -1902;
  if (connectivity != 4 && connectivity != 8) return -1903;
  if (min_area < 2 || min_area > (1 << 30)) return -1904;
  if (max_small < 1 || max_small > 65536) return -1905;
  if (workspace_bytes < 4 * L.words || ((uintptr_t)workspace & 3) || ((uintptr_t)stats & 3)) return -1906;
  const int HW = H * W, chunks = L.chunks;
  int* ws = reinterpret_cast<int*>(workspace);
  int* parent = ws + L.parent;
  int* aux = ws + L.aux;
  int* counts = ws + L.counts;
  int* total = ws + L.total;
  int* info = ws + L.info;
  int* votes = ws + L.votes;
  hipStream_t st = (hipStream_t)stream;
  const int conn8 = connectivity == 8;
  const unsigned long long kp = (unsigned long long)keep;
  const int cc_tx = (W + CC_TW - 1) / CC_TW, cc_ty = (H + CC_TH - 1) / CC_TH;
  const long rows_items = (long)(cc_ty - 1) * W, per_frame = L.border_items;
  const bool wide = (((uintptr_t)labels | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0 && W % CL_PPT == 0;
  const dim3 tiles((unsigned)(L.tpf * n)), per_chunk((unsigned)(chunks * n));
  stswin_zero_bytes(aux, sizeof(int) * (size_t)n * (size_t)HW, st);                     // (kernels, not hipMemsetAsync: see common.h)
  stswin_zero_bytes(votes, sizeof(int) * (size_t)n * (size_t)max_small * (size_t)nc, st);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(L.cc_tiles * n)), dim3(CC_THREADS), 0, st, labels, parent, H, W, nc, 0ull, conn8, cc_tx, cc_ty);
  if (per_frame > 0)
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((per_frame * n + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st, labels, parent, H,
                       W, nc, 0ull, conn8, rows_items, per_frame, per_frame * n);
  hipLaunchKernelGGL(cc_count_kernel, per_chunk, dim3(CC_THREADS), 0, st, parent, counts, HW, chunks);
  if (wide) hipLaunchKernelGGL(cl_area_kernel<true>, tiles, dim3(CL_THREADS), 0, st, (const int*)parent, aux, H, W, L.tiles_x, (int)L.tpf);
  else hipLaunchKernelGGL(cl_area_kernel<false>, tiles, dim3(CL_THREADS), 0, st, (const int*)parent, aux, H, W, L.tiles_x, (int)L.tpf);
  hipLaunchKernelGGL(cl_count_kernel, per_chunk, dim3(CC_THREADS), 0, st, labels, (const int*)parent, (const int*)aux, counts, HW, chunks, min_area,
                     kp);
  hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)n), dim3(CC_THREADS), 0, st, counts, total, chunks);
  hipLaunchKernelGGL(cl_number_kernel, per_chunk, dim3(CC_THREADS), 0, st, labels, (const int*)parent, aux, (const int*)counts, (const int*)total,
                     info, stats, HW, chunks, min_area, kp, max_small);
  if (wide)
    hipLaunchKernelGGL(cl_vote_kernel<true>, tiles, dim3(CL_THREADS), 0, st, labels, (const int*)parent, (const int*)aux, votes, H, W, nc, max_small,
                       L.tiles_x, (int)L.tpf);
  else
    hipLaunchKernelGGL(cl_vote_kernel<false>, tiles, dim3(CL_THREADS), 0, st, labels, (const int*)parent, (const int*)aux, votes, H, W, nc, max_small,
                       L.tiles_x, (int)L.tpf);
  hipLaunchKernelGGL(cl_resolve_kernel, dim3((unsigned)(L.resolve_bpf * n)), dim3(CC_THREADS), 0, st, labels, (const int*)votes, info, stats, HW, nc,
                     max_small, (int)L.resolve_bpf);
  if (wide)
    hipLaunchKernelGGL(cl_relabel_kernel<true>, tiles, dim3(CL_THREADS), 0, st, labels, (const int*)parent, (const int*)aux, (const int*)info, out, H,
                       W, max_small, L.tiles_x, (int)L.tpf);
  else
    hipLaunchKernelGGL(cl_relabel_kernel<false>, tiles, dim3(CL_THREADS), 0, st, labels, (const int*)parent, (const int*)aux, (const int*)info, out, H,
                       W, max_small, L.tiles_x, (int)L.tpf);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// The counts of the label launches, from a label map that already exists (VideoSegmenter(clean_area=A) scores the cleaned labels):
// counts[f][0 | 1 | 2][c] += |gt == c|, |labels == c|, |gt == c and labels == c| as upsample_argmax_kernel counts them, and / or
// cm[gt][labels] += 1 where both lie in [0, ncm) as upsample_argmax_cm_kernel does.  A workgroup takes LS_PIX consecutive pixels of one
// frame, counts them into LDS bins and adds every non-zero bin with one atomic.
#define LS_PIX 4096

template <bool CNT, bool CM>
__global__ __launch_bounds__(256) void labels_score_kernel(const unsigned char* __restrict__ labels, const long long* __restrict__ gt,
                                                           int* counts, unsigned long long* cm, int ncm, int nc, long HW,
                                                           int blocks_per_frame) {
  __shared__ int hist[CNT ? 3 * 64 : 1];
  __shared__ int hcm[CM ? 64 * 64 : 1];
  const int bins = ncm * ncm;
  if (CNT)
    for (int i = threadIdx.x; i < 3 * 64; i += 256) hist[i] = 0;
  if (CM)
    for (int i = threadIdx.x; i < bins; i += 256) hcm[i] = 0;
  __syncthreads();
  const int f = (int)(blockIdx.x / (unsigned)blocks_per_frame);
  const long p0 = (long)(blockIdx.x % (unsigned)blocks_per_frame) * LS_PIX;
  for (int k = 0; k < LS_PIX / 256; ++k) {
    const long px = p0 + k * 256 + threadIdx.x;
    if (px >= HW) break;
    const long long g = gt[(long)f * HW + px];
    const int l = (int)labels[(long)f * HW + px];
    if (CNT) {
      if (g >= 0 && g < 64) atomicAdd(&hist[(int)g], 1);
      if (l < nc) {
        atomicAdd(&hist[64 + l], 1);
        if (g == (long long)l) atomicAdd(&hist[128 + l], 1);
      }
    }
    if (CM && g >= 0 && g < ncm && l < ncm) atomicAdd(&hcm[(int)g * ncm + l], 1);
  }
  __syncthreads();
  if (CNT)
    for (int i = threadIdx.x; i < 3 * 64; i += 256) {
      const int k = i / 64, c = i % 64;
      if (c < nc && hist[i]) atomicAdd(counts + ((long)f * 3 + k) * nc + c, hist[i]);
    }
  if (CM)
    for (int i = threadIdx.x; i < bins; i += 256)
      if (hcm[i]) atomicAdd(cm + i, (unsigned long long)hcm[i]);
}

extern "C" int stswin_labels_score(const unsigned char* labels, const long long* gt, int* counts, unsigned long long* cm, int ncm, int n, int H,
                                   int W, int nc, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1910;
  if (labels == nullptr || gt == nullptr || (counts == nullptr && cm == nullptr)) return -1911;
  if (nc < 1 || nc > 64 || (cm != nullptr && (ncm < 1 || ncm > 64))) return -1912;
  if (((uintptr_t)gt & 7) || ((uintptr_t)counts & 3) || ((uintptr_t)cm & 7)) return -1913;
  const long HW = (long)H * W, bpf = (HW + LS_PIX - 1) / LS_PIX;
  if (bpf * n > 0x7fffffffL) return -1910;
  dim3 grid((unsigned)(bpf * n));
  hipStream_t st = (hipStream_t)stream;
#define LS_LAUNCH(CNT_, CM_) \
  hipLaunchKernelGGL((labels_score_kernel<CNT_, CM_>), grid, dim3(256), 0, st, labels, gt, counts, cm, cm ? ncm : 1, nc, HW, (int)bpf)
  if (counts != nullptr && cm != nullptr) LS_LAUNCH(true, true);
  else if (counts != nullptr) LS_LAUNCH(true, false);
  else LS_LAUNCH(false, true);
#undef LS_LAUNCH
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Instances followed from frame to frame (stswincl_amd/utils/instruments.py, InstanceTracker, states the result;
// VideoSegmenter(tracks=True)).  The state buffer, in int32 words (include/stswin_hip.h states it too):
//   [0] next id  [1] number of listed pairs  [2], [3] unused      cls[K], area[K], id[K] of the previous frame's instances (cls -1: takes
//   no part)      ov[K][K] overlap counts      list[K K] the pairs (i << 10 | j) whose count is non-zero      the previous component map,
//   16-byte aligned and padded with -1 to a multiple of four pixels
// Between two calls ov is all zero and the list is empty: a call's matching launch clears exactly the entries its overlap launch made.
//   1 trk_overlap_kernel  a thread reads four consecutive pixels of both maps (16-byte loads; 4-byte loads of a `components` that is
//                         not 16-byte aligned, and of a map's last pixels), writes the current ones over the previous ones and counts
//                         the pairs (i, j), both < K: equal pairs of its pixels in registers, the threads whose four pixels are one
//                         pair across the wave per distinct pair, everything into the workgroup's LDS table (slot j % TRK_SLOTS
//                         belongs to the first pair that claims it, others go to the global counter directly), which ends as one
//                         global atomic per slot in use.  The add that finds a zero lists the pair.  A wave without a pair - all
//                         background on either side - only copies.
//   2 trk_match_kernel    one workgroup: drops the listed pairs that are no candidates, then rounds of "every pair that is the most
//                         preferred remaining candidate of both its row and its column is matched" (compare-and-swap on the row's and
//                         the column's best in LDS; a turn ends or goes on against a strictly better pair) until a round matches
//                         nothing - the fixed point is the greedy matching - then ids, births by a scan over the ordinals, the new
//                         state, and the clearing of ov and the list.
// Integer atomics only: exact, whatever the order.  No kernel uses scratch memory or waits on another workgroup.
#define TRK_THREADS 256
#define TRK_VPT 2
#define TRK_SLOTS 64
#define TRK_MAXK 1024

struct TrkLayout {
  long cls, area, ids, ov, list, map, words;
};
static inline TrkLayout trk_layout(int H, int W, int K) {
  TrkLayout l;
  const long KK = (long)K * K;
  l.cls = 4, l.area = 4 + (long)K, l.ids = 4 + 2L * K, l.ov = 4 + 3L * K;
  l.list = l.ov + KK;
  l.map = (l.list + KK + 3) & ~3L;
  l.words = l.map + (((long)H * W + 3) & ~3L);
  return l;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_reset_kernel(int* __restrict__ s, long cls, long area, long ids, long ov, long map, long words) {
  for (long i = (long)blockIdx.x * TRK_THREADS + threadIdx.x; i < words; i += (long)gridDim.x * TRK_THREADS)
    s[i] = (i >= cls && i < area) || (i >= ids && i < ov) || i >= map ? -1 : 0;
}

__device__ __forceinline__ void trk_global(int* ov, int* list, int* npairs, int K, int key, unsigned c) {
  const int old = atomicAdd(ov + (long)(key >> 10) * K + (key & 1023), (int)c);
  if (old == 0) {                                         // (at most K K distinct pairs: the list of a reset state cannot overflow)
    const int at = atomicAdd(npairs, 1);
    if ((unsigned)at < (unsigned)(K * K)) list[at] = key;
  }
}

__device__ __forceinline__ void trk_add(int* tag, unsigned* cnt, int* ov, int* list, int* npairs, int K, int key, unsigned c) {
  const int slot = key & (TRK_SLOTS - 1);
  int owner = ((volatile int*)tag)[slot];
  if (owner == -1) {
    owner = atomicCAS(&tag[slot], -1, key);
    if (owner == -1) owner = key;
  }
  if (owner == key) atomicAdd(&cnt[slot], c);
  else trk_global(ov, list, npairs, K, key, c);
}

// COPY: the tracker without memory, which writes the current map over the previous one; !COPY: the memory tracker's first launch, which
// reads the memory map (slot indices) and writes nothing but the counts.
template <bool VEC, bool COPY>
__global__ __launch_bounds__(TRK_THREADS) void trk_overlap_kernel(const int* __restrict__ cur, int* __restrict__ prev, int* ov, int* list,
                                                                  int* npairs, long HW, int K) {
  __shared__ int tag[TRK_SLOTS];
  __shared__ unsigned cnt[TRK_SLOTS];
  if (threadIdx.x < TRK_SLOTS) tag[threadIdx.x] = -1, cnt[threadIdx.x] = 0u;
  __syncthreads();
  const long nvec = (HW + 3) >> 2;
  const int lane = (int)threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < TRK_VPT; ++it) {
    const long v = ((long)blockIdx.x * TRK_VPT + it) * TRK_THREADS + threadIdx.x;
    int4 c = make_int4(-1, -1, -1, -1), p = c;
    if (v < nvec) {
      const long p0 = 4 * v;
      p = *reinterpret_cast<const int4*>(prev + p0);           // (the state's map is padded: in range)
      if (VEC && p0 + 4 <= HW) {
        c = *reinterpret_cast<const int4*>(cur + p0);
      } else {
        if (p0 < HW) c.x = cur[p0];
        if (p0 + 1 < HW) c.y = cur[p0 + 1];
        if (p0 + 2 < HW) c.z = cur[p0 + 2];
        if (p0 + 3 < HW) c.w = cur[p0 + 3];
      }
      if (COPY) *reinterpret_cast<int4*>(prev + p0) = c;       // (each pixel's old value was read by this thread; the padding stays -1)
    }
    const unsigned uk = (unsigned)K;
    const int k0 = (unsigned)p.x < uk && (unsigned)c.x < uk ? (p.x << 10) | c.x : -1;
    const int k1 = (unsigned)p.y < uk && (unsigned)c.y < uk ? (p.y << 10) | c.y : -1;
    const int k2 = (unsigned)p.z < uk && (unsigned)c.z < uk ? (p.z << 10) | c.z : -1;
    const int k3 = (unsigned)p.w < uk && (unsigned)c.w < uk ? (p.w << 10) | c.w : -1;
    if (__ballot((k0 & k1 & k2 & k3) >= 0) == 0ull) continue;            // (wave-uniform) no pair in the wave's 256 pixels
    const bool full = k0 >= 0 && k0 == k1 && k1 == k2 && k2 == k3;
    if (!full) {                                                          // runs of equal pairs, left to right
      int rk = k0;
      unsigned rc = 1u;
      if (k1 == rk) ++rc;
      else {
        if (rk >= 0) trk_add(tag, cnt, ov, list, npairs, K, rk, rc);
        rk = k1, rc = 1u;
      }
      if (k2 == rk) ++rc;
      else {
        if (rk >= 0) trk_add(tag, cnt, ov, list, npairs, K, rk, rc);
        rk = k2, rc = 1u;
      }
      if (k3 == rk) ++rc;
      else {
        if (rk >= 0) trk_add(tag, cnt, ov, list, npairs, K, rk, rc);
        rk = k3, rc = 1u;
      }
      if (rk >= 0) trk_add(tag, cnt, ov, list, npairs, K, rk, rc);
    }
    unsigned long long todo = __ballot(full);                             // the threads of one pair, pair by pair (wave-uniform)
    while (todo) {
      const int first = __ffsll((long long)todo) - 1;
      const int k = __builtin_amdgcn_readlane(k0, first);
      const unsigned long long m = __ballot(full && k0 == k);
      todo &= ~m;
      if (lane == first) trk_add(tag, cnt, ov, list, npairs, K, k, 4u * (unsigned)__popcll(m));
    }
  }
  __syncthreads();
  if (threadIdx.x < TRK_SLOTS && tag[threadIdx.x] >= 0 && cnt[threadIdx.x]) trk_global(ov, list, npairs, K, tag[threadIdx.x], cnt[threadIdx.x]);
}

// a (overlap oa, union ua, key ka) is preferred to b: oa / ua > ob / ub as an exact int64 product (< 2^57), then the smaller (i, j)
__device__ __forceinline__ bool trk_better(long oa, long ua, long ka, long ob, long ub, long kb) {
  const long l = oa * ub, r = ob * ua;
  return l > r || (l == r && ka < kb);
}

// what breaks a tie between equally preferred pairs: the pair itself (i, j), or with BYID (the memory tracker, whose i is a slot)
// (the id of i's track, j)
template <bool BYID>
__device__ __forceinline__ long trk_rank(int key, const int* pids) {
  return BYID ? ((long)pids[key >> 10] << 10) | (key & 1023) : (long)key;
}

// the pair `key` becomes *best unless a better one holds it.  Each turn ends or continues against a strictly better holder.
template <bool BYID>
__device__ __forceinline__ void trk_contend(int* best, int key, long o, long u, const int* ov, const int* parea, const int* carea, const int* pids,
                                            int K) {
  int cur = *(volatile int*)best;
  for (;;) {
    if (cur >= 0) {
      const int ci = cur >> 10, cj = cur & 1023;
      const long co = ov[(long)ci * K + cj];
      if (!trk_better(o, u, trk_rank<BYID>(key, pids), co, (long)parea[ci] + carea[cj] - co, trk_rank<BYID>(cur, pids))) return;
    }
    const int old = atomicCAS(best, cur, key);
    if (old == cur) return;
    cur = old;
  }
}

__global__ __launch_bounds__(TRK_THREADS) void trk_match_kernel(const long long* __restrict__ rows, const int* __restrict__ total, int* hdr,
                                                                int* pcls, int* parea, int* pids, int* ov, int* list, int K, int min_iou,
                                                                int same_class, int min_area, int* __restrict__ ids, int* __restrict__ started) {
  __shared__ int ccls[TRK_MAXK], carea[TRK_MAXK], rbest[TRK_MAXK], cbest[TRK_MAXK], rmatch[TRK_MAXK], cmatch[TRK_MAXK];
  __shared__ unsigned red[4];
  __shared__ int changed;
  const int tid = (int)threadIdx.x;
  const int n = min(max(total[0], 0), K), np = min(max(hdr[1], 0), K * K), next = hdr[0];
  for (int j = tid; j < K; j += TRK_THREADS) {
    const long long a = j < n ? rows[(long)j * 12 + 2] : 0ll;
    const bool part = j < n && a >= (long long)min_area;
    ccls[j] = part ? (int)rows[(long)j * 12] : -1;
    carea[j] = part ? (int)a : 0;
    rmatch[j] = cmatch[j] = -1;
  }
  __syncthreads();
  for (int p = tid; p < np; p += TRK_THREADS) {               // the listed pairs that are no candidates leave the list
    const int key = list[p], i = key >> 10, j = key & 1023;
    if (key < 0 || i >= K || j >= K) {                         // (only a state that was never reset holds such a key)
      list[p] = -1;
      continue;
    }
    const long o = ov[(long)i * K + j];
    const int pc = pcls[i], cc = ccls[j];
    bool ok = pc >= 0 && cc >= 0 && (!same_class || pc == cc);
    if (ok) ok = 1000l * o >= (long)min_iou * ((long)parea[i] + carea[j] - o);
    if (!ok) ov[(long)i * K + j] = 0, list[p] = -1;
  }
  for (;;) {
    for (int j = tid; j < K; j += TRK_THREADS) rbest[j] = cbest[j] = -1;
    if (tid == 0) changed = 0;
    __syncthreads();
    for (int p = tid; p < np; p += TRK_THREADS) {
      const int key = list[p];
      if (key < 0) continue;
      const int i = key >> 10, j = key & 1023;
      if (rmatch[i] >= 0 || cmatch[j] >= 0) {                 // matched, or beaten for good: done with
        ov[(long)i * K + j] = 0, list[p] = -1;
        continue;
      }
      const long o = ov[(long)i * K + j], u = (long)parea[i] + carea[j] - o;
      trk_contend<false>(rbest + i, key, o, u, ov, parea, carea, pids, K);
      trk_contend<false>(cbest + j, key, o, u, ov, parea, carea, pids, K);
    }
    __syncthreads();
    for (int p = tid; p < np; p += TRK_THREADS) {
      const int key = list[p];
      if (key < 0) continue;
      const int i = key >> 10, j = key & 1023;
      if (rbest[i] == key && cbest[j] == key) rmatch[i] = j, cmatch[j] = i, changed = 1;
    }
    __syncthreads();
    const int c = changed;
    __syncthreads();
    if (!c) break;
  }
  for (int p = tid; p < np; p += TRK_THREADS) {               // (none is left at the fixed point; the state's invariant does not rest on it)
    const int key = list[p];
    if (key >= 0) ov[(long)(key >> 10) * K + (key & 1023)] = 0, list[p] = -1;
  }
  unsigned carry = 0;                                          // births: the unmatched participants, numbered in ascending j
  for (int base = 0; base < K; base += TRK_THREADS) {
    const int j = base + tid;
    const int m = j < K ? cmatch[j] : -1;
    const unsigned b = j < K && ccls[j] >= 0 && m < 0 ? 1u : 0u;
    const unsigned incl = cc_block_scan(b, red);
    if (j < K) rbest[j] = m >= 0 ? pids[m] : b ? next + (int)(carry + incl - 1u) : -1;
    carry += red[0] + red[1] + red[2] + red[3];
  }
  __syncthreads();                                             // (every previous id has been read)
  for (int j = tid; j < K; j += TRK_THREADS) {
    const int id = rbest[j];
    ids[j] = id;
    pids[j] = id, pcls[j] = ccls[j], parea[j] = carea[j];
  }
  if (tid == 0) hdr[0] = next + (int)carry, hdr[1] = 0, started[0] = next + (int)carry;
}

extern "C" long stswin_track_state_bytes(int H, int W, int K) {
  if (H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1840;
  if (K < 1 || K > TRK_MAXK) return -1841;
  return 4 * trk_layout(H, W, K).words;
}

extern "C" int stswin_track_reset(void* state, long state_bytes, int H, int W, int K, void* stream) {
  if (H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1840;
  if (K < 1 || K > TRK_MAXK) return -1841;
  if (state == nullptr) return -1842;
  const TrkLayout l = trk_layout(H, W, K);
  if (state_bytes < 4 * l.words || ((uintptr_t)state & 15)) return -1843;
  long blocks = (l.words + TRK_THREADS - 1) / TRK_THREADS;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(trk_reset_kernel, dim3((unsigned)blocks), dim3(TRK_THREADS), 0, (hipStream_t)stream, reinterpret_cast<int*>(state), l.cls,
                     l.area, l.ids, l.ov, l.map, l.words);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_track_instances(const int* components, const long long* rows, const int* total, void* state, long state_bytes, int H,
                                      int W, int K, int min_iou, int same_class, int min_area, int* ids, int* started, void* stream) {
  if (H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1840;
  if (K < 1 || K > TRK_MAXK) return -1841;
  if (components == nullptr || rows == nullptr || total == nullptr || state == nullptr || ids == nullptr || started == nullptr) return -1842;
  const TrkLayout l = trk_layout(H, W, K);
  if (state_bytes < 4 * l.words || ((uintptr_t)state & 15)) return -1843;
  if (((uintptr_t)components & 3) || ((uintptr_t)rows & 7) || ((uintptr_t)total & 3) || ((uintptr_t)ids & 3) || ((uintptr_t)started & 3)) return -1844;
  if (min_iou < 0 || min_iou > 1000 || (same_class != 0 && same_class != 1) || min_area < 1) return -1845;
  hipStream_t st = (hipStream_t)stream;
  int* s = reinterpret_cast<int*>(state);
  const long HW = (long)H * W, nvec = (HW + 3) >> 2;
  const unsigned blocks = (unsigned)((nvec + TRK_THREADS * TRK_VPT - 1) / (TRK_THREADS * TRK_VPT));       // <= 2^17
  if ((uintptr_t)components & 15)
    hipLaunchKernelGGL((trk_overlap_kernel<false, true>), dim3(blocks), dim3(TRK_THREADS), 0, st, components, s + l.map, s + l.ov, s + l.list, s + 1, HW, K);
  else
    hipLaunchKernelGGL((trk_overlap_kernel<true, true>), dim3(blocks), dim3(TRK_THREADS), 0, st, components, s + l.map, s + l.ov, s + l.list, s + 1, HW, K);
  hipLaunchKernelGGL(trk_match_kernel, dim3(1), dim3(TRK_THREADS), 0, st, rows, total, s, s + l.cls, s + l.area, s + l.ids, s + l.ov, s + l.list,
                     K, min_iou, same_class, min_area, ids, started);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// The tracker with a memory (stswincl_amd/utils/instruments.py, MemoryTracker, states the result; VideoSegmenter(tracks=True,
// track_max_gap=g)): a track that no instance was matched to stays alive for up to max_gap frames, and instances are matched against
// the mask it had when it was last seen.  The live tracks sit in K slots - which slot a track has shows in no output - and the memory
// map holds, per pixel, the slot of the track it is remembered for.  The state buffer, in int32 words (include/stswin_hip.h too):
//   [0] next id  [1] number of listed pairs  [2], [3] unused      cls[K] (-1: a free slot), area[K], id[K], age[K] of the slots
//   slot_of[K] the slot of each current ordinal (-1: takes no part)      keep[K] per slot: 1 if its remembered pixels stay
//   ov[K][K] overlap counts (slot, ordinal)      list[K K] the pairs (slot << 10 | j) whose count is non-zero      the memory map,
//   16-byte aligned and padded with -1 to a multiple of four pixels
// Between two calls ov is all zero and the list is empty, as above.
//   1 trk_overlap_kernel<.., false>  the overlap pass above over the memory map and the component map; it writes neither
//   2 trk_mem_match_kernel           one workgroup: the candidate filter and the rounds of trk_match_kernel with the track's id in the
//                                    tie-break; ids and started; then per slot matched (takes the instance's class and area, age 0),
//                                    aged or ended; if more than K tracks would live, the lost ones are ranked by (age descending,
//                                    id ascending) among themselves and the first ones end; births take the free slots in ascending
//                                    order of both; slot_of and keep for the third launch; ov and the list cleared
//   3 trk_commit_kernel              four pixels per thread, slot_of and keep in LDS: mem = the pixel's instance takes part ?
//                                    slot_of[comp] : (mem >= 0 and keep[mem] ? mem : -1), stored where it changes anything
// Integer atomics only.  No kernel uses scratch memory or waits on another workgroup.
#define TRK_CVPT 4

struct TrkMemLayout {
  long cls, area, ids, age, slot_of, keep, ov, list, map, words;
};
static inline TrkMemLayout trk_mem_layout(int H, int W, int K) {
  TrkMemLayout l;
  const long KK = (long)K * K;
  l.cls = 4, l.area = 4 + (long)K, l.ids = 4 + 2L * K, l.age = 4 + 3L * K, l.slot_of = 4 + 4L * K, l.keep = 4 + 5L * K, l.ov = 4 + 6L * K;
  l.list = l.ov + KK;
  l.map = (l.list + KK + 3) & ~3L;
  l.words = l.map + (((long)H * W + 3) & ~3L);
  return l;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_mem_reset_kernel(int* __restrict__ s, long cls, long area, long ids, long age, long slot_of,
                                                                    long keep, long map, long words) {
  for (long i = (long)blockIdx.x * TRK_THREADS + threadIdx.x; i < words; i += (long)gridDim.x * TRK_THREADS)
    s[i] = (i >= cls && i < area) || (i >= ids && i < age) || (i >= slot_of && i < keep) || i >= map ? -1 : 0;
}

__global__ __launch_bounds__(TRK_THREADS) void trk_mem_match_kernel(const long long* __restrict__ rows, const int* __restrict__ total, int* hdr,
                                                                    int* pcls, int* parea, int* pids, int* page, int* slot_of, int* keep,
                                                                    int* ov, int* list, int K, int max_gap, int min_iou, int same_class,
                                                                    int min_area, int* __restrict__ ids, int* __restrict__ started) {
  __shared__ int ccls[TRK_MAXK], carea[TRK_MAXK], rbest[TRK_MAXK], cbest[TRK_MAXK], rmatch[TRK_MAXK], cmatch[TRK_MAXK];
  __shared__ long lostkey[TRK_MAXK];       // a lost slot: age << 32 | (2^31 - 1 - id), the larger one ends first; 0: not lost
  __shared__ int ends[TRK_MAXK], freel[TRK_MAXK];
  __shared__ unsigned red[4];
  __shared__ int changed, nkept[2];
  const int tid = (int)threadIdx.x;
  const int n = min(max(total[0], 0), K), np = min(max(hdr[1], 0), K * K), next = hdr[0];
  for (int j = tid; j < K; j += TRK_THREADS) {
    const long long a = j < n ? rows[(long)j * 12 + 2] : 0ll;
    const bool part = j < n && a >= (long long)min_area;
    ccls[j] = part ? (int)rows[(long)j * 12] : -1;
    carea[j] = part ? (int)a : 0;
    rmatch[j] = cmatch[j] = -1;
  }
  if (tid < 2) nkept[tid] = 0;
  __syncthreads();
  for (int p = tid; p < np; p += TRK_THREADS) {               // the listed pairs that are no candidates leave the list
    const int key = list[p], i = key >> 10, j = key & 1023;
    if (key < 0 || i >= K || j >= K) {                         // (only a state that was never reset holds such a key)
      list[p] = -1;
      continue;
    }
    const long o = ov[(long)i * K + j];
    const int pc = pcls[i], cc = ccls[j];
    bool ok = pc >= 0 && cc >= 0 && (!same_class || pc == cc);
    if (ok) ok = 1000l * o >= (long)min_iou * ((long)parea[i] + carea[j] - o);
    if (!ok) ov[(long)i * K + j] = 0, list[p] = -1;
  }
  for (;;) {
    for (int j = tid; j < K; j += TRK_THREADS) rbest[j] = cbest[j] = -1;
    if (tid == 0) changed = 0;
    __syncthreads();
    for (int p = tid; p < np; p += TRK_THREADS) {
      const int key = list[p];
      if (key < 0) continue;
      const int i = key >> 10, j = key & 1023;
      if (rmatch[i] >= 0 || cmatch[j] >= 0) {                 // matched, or beaten for good: done with
        ov[(long)i * K + j] = 0, list[p] = -1;
        continue;
      }
      const long o = ov[(long)i * K + j], u = (long)parea[i] + carea[j] - o;
      trk_contend<true>(rbest + i, key, o, u, ov, parea, carea, pids, K);
      trk_contend<true>(cbest + j, key, o, u, ov, parea, carea, pids, K);
    }
    __syncthreads();
    for (int p = tid; p < np; p += TRK_THREADS) {
      const int key = list[p];
      if (key < 0) continue;
      const int i = key >> 10, j = key & 1023;
      if (rbest[i] == key && cbest[j] == key) rmatch[i] = j, cmatch[j] = i, changed = 1;
    }
    __syncthreads();
    const int c = changed;
    __syncthreads();
    if (!c) break;
  }
  for (int p = tid; p < np; p += TRK_THREADS) {               // (none is left at the fixed point; the state's invariant does not rest on it)
    const int key = list[p];
    if (key >= 0) ov[(long)(key >> 10) * K + (key & 1023)] = 0, list[p] = -1;
  }
  unsigned births = 0;                                         // births: the unmatched participants, numbered in ascending j
  for (int base = 0; base < K; base += TRK_THREADS) {
    const int j = base + tid;
    const int m = j < K ? cmatch[j] : -1;
    const unsigned b = j < K && ccls[j] >= 0 && m < 0 ? 1u : 0u;
    const unsigned incl = cc_block_scan(b, red);
    if (j < K) {
      rbest[j] = m >= 0 ? pids[m] : b ? next + (int)(births + incl - 1u) : -1;      // the id of ordinal j ...
      cbest[j] = b ? (int)(births + incl - 1u) : -1;                                 // ... and which birth it is
    }
    births += red[0] + red[1] + red[2] + red[3];
  }
  for (int i = tid; i < K; i += TRK_THREADS) {                 // the slots: matched, lost (age 1 .. max_gap) or over
    const bool live = pcls[i] >= 0, matched = live && rmatch[i] >= 0;
    const int age = live && !matched ? page[i] + 1 : 0;
    const bool lost = age >= 1 && age <= max_gap;
    lostkey[i] = lost ? ((long)age << 32) | (long)(0x7fffffff - pids[i]) : 0l;
    ends[i] = 0;
    if (matched) atomicAdd(&nkept[0], 1);
    if (lost) atomicAdd(&nkept[1], 1);
  }
  __syncthreads();
  const int over = nkept[0] + nkept[1] + (int)births - K;      // more than K tracks: the `over` oldest lost ones end, the smaller id first
  if (over > 0) {
    for (int i = tid; i < K; i += TRK_THREADS) {
      const long key = lostkey[i];
      if (key == 0l) continue;
      int before = 0;
#pragma unroll 8
      for (int o = 0; o < K; ++o) before += lostkey[o] > key ? 1 : 0;
      ends[i] = before < over ? 1 : 0;
    }
    __syncthreads();
  }
  unsigned nfree = 0;                                          // the slots' new state; the free ones, listed in ascending order
  for (int base = 0; base < K; base += TRK_THREADS) {
    const int i = base + tid;
    unsigned f = 0u;
    if (i < K) {
      const int j = pcls[i] >= 0 ? rmatch[i] : -1;
      const bool stays = lostkey[i] != 0l && !ends[i];
      if (j >= 0) pcls[i] = ccls[j], parea[i] = carea[j], page[i] = 0, keep[i] = 0;
      else if (stays) page[i] = (int)(lostkey[i] >> 32), keep[i] = 1;
      else pcls[i] = -1, parea[i] = 0, pids[i] = -1, page[i] = 0, keep[i] = 0, f = 1u;
    }
    const unsigned incl = cc_block_scan(f, red);
    if (f) freel[nfree + incl - 1u] = i;
    nfree += red[0] + red[1] + red[2] + red[3];
  }
  __syncthreads();                                             // (the free list is complete, every slot's state is written)
  for (int j = tid; j < K; j += TRK_THREADS) {
    const int id = rbest[j], b = cbest[j];
    int slot = cmatch[j];
    if (b >= 0) {                                              // (a birth always finds a free slot: at most K tracks live)
      slot = (unsigned)b < nfree ? freel[b] : -1;
      if (slot >= 0) pcls[slot] = ccls[j], parea[slot] = carea[j], pids[slot] = id, page[slot] = 0;
    }
    ids[j] = id;
    slot_of[j] = ccls[j] >= 0 ? slot : -1;
  }
  if (tid == 0) hdr[0] = next + (int)births, hdr[1] = 0, started[0] = next + (int)births;
}

template <bool VEC>
__global__ __launch_bounds__(TRK_THREADS) void trk_commit_kernel(const int* __restrict__ cur, int* __restrict__ mem, const int* __restrict__ slot_of,
                                                                 const int* __restrict__ keep, long HW, int K) {
  __shared__ int so[TRK_MAXK], kp[TRK_MAXK];
  for (int j = (int)threadIdx.x; j < K; j += TRK_THREADS) so[j] = slot_of[j], kp[j] = keep[j];
  __syncthreads();
  const long nvec = (HW + 3) >> 2;
  const unsigned uk = (unsigned)K;
#pragma unroll
  for (int it = 0; it < TRK_CVPT; ++it) {
    const long v = ((long)blockIdx.x * TRK_CVPT + it) * TRK_THREADS + threadIdx.x;
    if (v >= nvec) continue;
    const long p0 = 4 * v;
    int4 c = make_int4(-1, -1, -1, -1);
    const int4 m = *reinterpret_cast<const int4*>(mem + p0);   // (the state's map is padded: in range)
    if (VEC && p0 + 4 <= HW) {
      c = *reinterpret_cast<const int4*>(cur + p0);
    } else {
      if (p0 < HW) c.x = cur[p0];
      if (p0 + 1 < HW) c.y = cur[p0 + 1];
      if (p0 + 2 < HW) c.z = cur[p0 + 2];
      if (p0 + 3 < HW) c.w = cur[p0 + 3];
    }
    int4 r;                                                    // (the padding has c = -1 and m = -1: it stays -1)
    int s;
    s = (unsigned)c.x < uk ? so[c.x] : -1, r.x = s >= 0 ? s : (unsigned)m.x < uk && kp[m.x] ? m.x : -1;
    s = (unsigned)c.y < uk ? so[c.y] : -1, r.y = s >= 0 ? s : (unsigned)m.y < uk && kp[m.y] ? m.y : -1;
    s = (unsigned)c.z < uk ? so[c.z] : -1, r.z = s >= 0 ? s : (unsigned)m.z < uk && kp[m.z] ? m.z : -1;
    s = (unsigned)c.w < uk ? so[c.w] : -1, r.w = s >= 0 ? s : (unsigned)m.w < uk && kp[m.w] ? m.w : -1;
    if (r.x != m.x || r.y != m.y || r.z != m.z || r.w != m.w) *reinterpret_cast<int4*>(mem + p0) = r;
  }
}

static int trk_mem_shape(int H, int W, int K) {
  if (H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1860;
  if (K < 1 || K > TRK_MAXK) return -1861;
  return 0;
}

extern "C" long stswin_track_memory_state_bytes(int H, int W, int K) {
  const int e = trk_mem_shape(H, W, K);
  return e ? e : 4 * trk_mem_layout(H, W, K).words;
}

extern "C" int stswin_track_memory_reset(void* state, long state_bytes, int H, int W, int K, void* stream) {
  const int e = trk_mem_shape(H, W, K);
  if (e) return e;
  if (state == nullptr) return -1862;
  const TrkMemLayout l = trk_mem_layout(H, W, K);
  if (state_bytes < 4 * l.words || ((uintptr_t)state & 15)) return -1863;
  long blocks = (l.words + TRK_THREADS - 1) / TRK_THREADS;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(trk_mem_reset_kernel, dim3((unsigned)blocks), dim3(TRK_THREADS), 0, (hipStream_t)stream, reinterpret_cast<int*>(state), l.cls,
                     l.area, l.ids, l.age, l.slot_of, l.keep, l.map, l.words);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_track_memory(const int* components, const long long* rows, const int* total, void* state, long state_bytes, int H, int W,
                                   int K, int max_gap, int min_iou, int same_class, int min_area, int* ids, int* started, void* stream) {
  const int e = trk_mem_shape(H, W, K);
  if (e) return e;
  if (components == nullptr || rows == nullptr || total == nullptr || state == nullptr || ids == nullptr || started == nullptr) return -1862;
  const TrkMemLayout l = trk_mem_layout(H, W, K);
  if (state_bytes < 4 * l.words || ((uintptr_t)state & 15)) return -1863;
  if (((uintptr_t)components & 3) || ((uintptr_t)rows & 7) || ((uintptr_t)total & 3) || ((uintptr_t)ids & 3) || ((uintptr_t)started & 3)) return -1864;
  if (min_iou < 0 || min_iou > 1000 || (same_class != 0 && same_class != 1) || min_area < 1) return -1865;
  if (max_gap < 0 || max_gap > 1000000) return -1866;
  hipStream_t st = (hipStream_t)stream;
  int* s = reinterpret_cast<int*>(state);
  const long HW = (long)H * W, nvec = (HW + 3) >> 2;
  const bool vec = ((uintptr_t)components & 15) == 0;
  const unsigned blocks = (unsigned)((nvec + TRK_THREADS * TRK_VPT - 1) / (TRK_THREADS * TRK_VPT));       // <= 2^17
  const unsigned cblocks = (unsigned)((nvec + TRK_THREADS * TRK_CVPT - 1) / (TRK_THREADS * TRK_CVPT));
  if (vec)
    hipLaunchKernelGGL((trk_overlap_kernel<true, false>), dim3(blocks), dim3(TRK_THREADS), 0, st, components, s + l.map, s + l.ov, s + l.list, s + 1, HW, K);
  else
    hipLaunchKernelGGL((trk_overlap_kernel<false, false>), dim3(blocks), dim3(TRK_THREADS), 0, st, components, s + l.map, s + l.ov, s + l.list, s + 1, HW, K);
  hipLaunchKernelGGL(trk_mem_match_kernel, dim3(1), dim3(TRK_THREADS), 0, st, rows, total, s, s + l.cls, s + l.area, s + l.ids, s + l.age,
                     s + l.slot_of, s + l.keep, s + l.ov, s + l.list, K, max_gap, min_iou, same_class, min_area, ids, started);
  if (vec)
    hipLaunchKernelGGL(trk_commit_kernel<true>, dim3(cblocks), dim3(TRK_THREADS), 0, st, components, s + l.map, s + l.slot_of, s + l.keep, HW, K);
  else
    hipLaunchKernelGGL(trk_commit_kernel<false>, dim3(cblocks), dim3(TRK_THREADS), 0, st, components, s + l.map, s + l.slot_of, s + l.keep, HW, K);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Run-length masks (stswincl_amd/utils/rle.py, encode, states the result; VideoSegmenter(masks=...)): a uint8 label map or an int32
// component map [n][H][W] -> per frame the runs (p, v) of its column-major reading p = x H + y, sorted by p, the first `cap` of them.
// Pixel (y, x) starts a run iff it differs from the pixel above it, for y = 0 from the last pixel of the column to its left, and
// p = 0 always does: the flags come from row-major reads although the order of the result is column-major.  The height is cut into
// segments of RLE_SH rows, the width into bands of RLE_TW columns; a thread owns V adjacent columns of one segment (V = RLE_V = 16
// uint8 or 4 int32: 16 bytes per row) and walks the segment's rows with the previous row in registers, RLE_ROWS loads in flight.
//   1 rle_walk_kernel<.., false>  counts the starts per (column, segment) into a table laid out [W][S]: column-major run order is
//                                 linear table order
//   2 rle_scan_kernel             one workgroup per frame: exclusive scan of the table (in place, through LDS) and count[f]
//   3 rle_walk_kernel<.., true>   the same walk with a running rank per column that starts from the table's offset: stores (p, v)
//                                 where the rank is below cap; the frame's threads also zero runs from min(count, cap) on
// WIDE (map 16-byte aligned and a row a multiple of 16 bytes) takes one 16-byte load per row, anything else element loads.  No atomics:
// every word of the result has one writer.  No kernel uses scratch memory or waits on another workgroup.
#define RLE_SH 32
#define RLE_TW 256
#define RLE_V 16
#define RLE_THREADS 256
#define RLE_ROWS 4
#define RLE_SCAN_THREADS 1024
#define RLE_SCAN_ITEMS 8

template <int EB>
__device__ __forceinline__ int rle_value(const uint4& v, int i) {               // (i is a constant after unrolling)
  if (EB == 4) return (int)(i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w);
  return (int)lm_byte(v, i);
}

// elements xs .. xs + V - 1 of the row at `row`, zero where the column is outside 0 .. W - 1 (xs may be -1)
template <int EB>
__device__ __forceinline__ uint4 rle_gather(const unsigned char* __restrict__ row, int xs, int W) {
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (EB == 4) {
    const unsigned* r = reinterpret_cast<const unsigned*>(row);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (xs + i >= 0 && xs + i < W) w[i] = r[xs + i];
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (xs + i >= 0 && xs + i < W) w[i >> 2] |= (unsigned)row[xs + i] << (8 * (i & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int EB, bool WIDE>
__device__ __forceinline__ uint4 rle_load(const unsigned char* __restrict__ row, int x0, int W) {
  if (WIDE) return *reinterpret_cast<const uint4*>(row + (long)x0 * EB);
  return rle_gather<EB>(row, x0, W);
}

template <int EB, bool WIDE, bool WRITE>
__global__ __launch_bounds__(RLE_THREADS) void rle_walk_kernel(const unsigned char* __restrict__ map, int* table, int* __restrict__ runs,
                                                               const int* __restrict__ count, int H, int W, int S, int cap, int bands,
                                                               int segblocks) {
  constexpr int V = EB == 1 ? RLE_V : 4, GPB = RLE_TW / V, SPB = RLE_THREADS / GPB;
  unsigned b = blockIdx.x;
  const int band = (int)(b % (unsigned)bands);
  b /= (unsigned)bands;
  const int sb = (int)(b % (unsigned)segblocks), f = (int)(b / (unsigned)segblocks);
  const int s = sb * SPB + (int)threadIdx.x / GPB, x0 = band * RLE_TW + ((int)threadIdx.x % GPB) * V;
  int* fr = runs + 2 * (long)f * cap;             // (p, v) pairs; runs is only known to be 4-byte aligned: word stores
  if (WRITE) {                                   // the tail: every thread of the frame's workgroups takes its share
    const int R = count[f];
    const long tpf = (long)bands * segblocks * RLE_THREADS;
    for (long i = (long)min(R, cap) + ((long)sb * bands + band) * RLE_THREADS + threadIdx.x; i < cap; i += tpf) fr[2 * i] = 0, fr[2 * i + 1] = 0;
  }
  if (s >= S || x0 >= W) return;
  int* tb = table + (long)f * W * S;
  int rank[V];
#pragma unroll
  for (int i = 0; i < V; ++i) rank[i] = WRITE && x0 + i < W ? tb[(x0 + i) * S + s] : 0;
  const long pitch = (long)W * EB;
  const unsigned char* fm = map + (long)f * H * pitch;
  const int y0 = s * RLE_SH, y1 = min(H, y0 + RLE_SH);
  const unsigned colmask = W - x0 >= V ? (1u << V) - 1u : (1u << (W - x0)) - 1u;
  // the row above the segment; above row 0 every column sees the last pixel of the column to its left
  uint4 prev = y0 > 0 ? rle_load<EB, WIDE>(fm + (y0 - 1) * pitch, x0, W) : rle_gather<EB>(fm + (H - 1) * pitch, x0 - 1, W);
  for (int y = y0; y < y1; y += RLE_ROWS) {
    uint4 cur[RLE_ROWS];
#pragma unroll
    for (int r = 0; r < RLE_ROWS; ++r)
      cur[r] = y + r < y1 ? rle_load<EB, WIDE>(fm + (y + r) * pitch, x0, W) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int r = 0; r < RLE_ROWS; ++r) {
      if (y + r >= y1) continue;
      const uint4 c = cur[r];
      unsigned m = 0;
      if (((c.x ^ prev.x) | (c.y ^ prev.y) | (c.z ^ prev.z) | (c.w ^ prev.w)) != 0u) {
#pragma unroll
        for (int i = 0; i < V; ++i)
          if (rle_value<EB>(c, i) != rle_value<EB>(prev, i)) m |= 1u << i;
        m &= colmask;
      }
      if (y + r == 0 && x0 == 0) m |= 1u;        // p = 0 starts a run whatever the map's last pixel holds
      if (m) {
#pragma unroll
        for (int i = 0; i < V; ++i)
          if (m >> i & 1u) {
            if (WRITE && rank[i] < cap) fr[2 * (long)rank[i]] = (x0 + i) * H + y + r, fr[2 * (long)rank[i] + 1] = rle_value<EB>(c, i);
            ++rank[i];
          }
      }
      prev = c;
    }
  }
  if (!WRITE) {
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (x0 + i < W) tb[(x0 + i) * S + s] = rank[i];
  }
}

// One workgroup of 16 waves: a round scans 1024 x 8 entries.  The entries come in and go out through LDS so that the lanes of a wave
// touch consecutive words of the table (a thread that read its own 8 consecutive entries from memory would cost a cache-line access
// per lane and entry, and the one compute unit's 2 W S of them were the longest part of the call); in LDS entry i lies at i + i / 8, so
// that the threads' runs of 8 start 9 words apart and hit distinct banks.  A thread sums its 8 entries, the waves scan the sums with
// shuffles, the 16 wave totals go through LDS.
__global__ __launch_bounds__(RLE_SCAN_THREADS) void rle_scan_kernel(int* table, int* __restrict__ count, int entries) {
  constexpr int ROUND = RLE_SCAN_THREADS * RLE_SCAN_ITEMS;
  __shared__ unsigned buf[ROUND + ROUND / RLE_SCAN_ITEMS];
  __shared__ unsigned red[RLE_SCAN_THREADS / 64];
  int* t = table + (long)blockIdx.x * entries;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* mine = buf + tid * (RLE_SCAN_ITEMS + 1);
  unsigned carry = 0;
  for (int base = 0; base < entries; base += ROUND) {
#pragma unroll
    for (int k = 0; k < RLE_SCAN_ITEMS; ++k) {
      const int i = k * RLE_SCAN_THREADS + tid;
      buf[i + i / RLE_SCAN_ITEMS] = base + i < entries ? (unsigned)t[base + i] : 0u;
    }
    __syncthreads();
    unsigned v[RLE_SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int k = 0; k < RLE_SCAN_ITEMS; ++k) {
      v[k] = mine[k];
      sum += v[k];
    }
    unsigned incl = sum;                         // inclusive over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;                // the totals of the waves in front, and of all of them
#pragma unroll
    for (int k = 0; k < RLE_SCAN_THREADS / 64; ++k) {
      const unsigned r = red[k];
      if (k < wave) before += r;
      all += r;
    }
    unsigned o = carry + before + incl - sum;
#pragma unroll
    for (int k = 0; k < RLE_SCAN_ITEMS; ++k) {
      mine[k] = o;
      o += v[k];
    }
    carry += all;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RLE_SCAN_ITEMS; ++k) {
      const int i = k * RLE_SCAN_THREADS + tid;
      if (base + i < entries) t[base + i] = (int)buf[i + i / RLE_SCAN_ITEMS];
    }
    __syncthreads();                             // (buf and red are free for the next round)
  }
  if (threadIdx.x == 0) count[blockIdx.x] = (int)carry;
}

extern "C" int stswin_rle_geometry(int which) { return which == 0 ? RLE_SH : which == 1 ? RLE_TW : which == 2 ? RLE_V : -1; }

extern "C" long stswin_rle_encode_scratch(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1850;
  return 4 * (long)n * W * ((H + RLE_SH - 1) / RLE_SH);               // the table [n][W][S]
}

template <int EB, bool WIDE>
static void rle_launch(const unsigned char* map, int* table, int* runs, int* count, int n, int H, int W, int S, int cap, int bands,
                       int segblocks, hipStream_t st) {
  const dim3 grid((unsigned)((long)bands * segblocks * n));
  hipLaunchKernelGGL((rle_walk_kernel<EB, WIDE, false>), grid, dim3(RLE_THREADS), 0, st, map, table, runs, (const int*)count, H, W, S, cap, bands,
                     segblocks);
  hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)n), dim3(RLE_SCAN_THREADS), 0, st, table, count, W * S);
  hipLaunchKernelGGL((rle_walk_kernel<EB, WIDE, true>), grid, dim3(RLE_THREADS), 0, st, map, table, runs, (const int*)count, H, W, S, cap, bands,
                     segblocks);
}

extern "C" int stswin_rle_encode(const void* map, int elem_bytes, int* runs, int* count, int n, int H, int W, int cap, void* workspace,
                                 long workspace_bytes, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1850;
  if (map == nullptr || runs == nullptr || count == nullptr || workspace == nullptr) return -1851;
  if (elem_bytes != 1 && elem_bytes != 4) return -1852;
  if (cap < 1 || cap > 1048576) return -1853;
  if (workspace_bytes < stswin_rle_encode_scratch(n, H, W) || ((uintptr_t)workspace & 3)) return -1854;
  if (((uintptr_t)map & (uintptr_t)(elem_bytes - 1)) || ((uintptr_t)runs & 3) || ((uintptr_t)count & 3)) return -1855;
  const int S = (H + RLE_SH - 1) / RLE_SH, bands = (W + RLE_TW - 1) / RLE_TW;
  const int spb = RLE_THREADS / (RLE_TW / (elem_bytes == 1 ? RLE_V : 4)), segblocks = (S + spb - 1) / spb;
  if ((long)bands * segblocks * n > 0x7fffffffL) return -1850;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* m = reinterpret_cast<const unsigned char*>(map);
  int* table = reinterpret_cast<int*>(workspace);
  const bool wide = ((uintptr_t)map & 15) == 0 && ((long)W * elem_bytes) % 16 == 0;
  if (elem_bytes == 1) {
    if (wide) rle_launch<1, true>(m, table, runs, count, n, H, W, S, cap, bands, segblocks, st);
    else rle_launch<1, false>(m, table, runs, count, n, H, W, S, cap, bands, segblocks, st);
  } else {
    if (wide) rle_launch<4, true>(m, table, runs, count, n, H, W, S, cap, bands, segblocks, st);
    else rle_launch<4, false>(m, table, runs, count, n, H, W, S, cap, bands, segblocks, st);
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Boundary scores (stswincl_amd/utils/boundary.py, boundary_counts, states the result; VideoSegmenter(boundary=...)): per class the
// exact squared Euclidean distance from every contour pixel of one label map to the nearest contour pixel of the other, as counts
// per ceil(distance) and the maximum, in both directions.  Five launches whatever nc and the maps hold:
//   1 bnd_fill_kernel    out: rows of skipped classes 0, elsewhere count 0, maximum -1, histogram 0
//   2 bnd_mark_kernel    both maps -> code maps uint8 [2][n][H][W]: the pixel's class where it is a contour pixel of a scored class
//                        (a 4-neighbour holds another value, or lies outside the image), BND_NONE elsewhere
//   3 bnd_mask_kernel    per map, column and segment of BND_SEG rows the classes with a contour pixel there, one bit each: the table
//                        uint64 [2][n][S][W] that lets the next pass find the nearest contour row outside a segment without walking
//                        the column
//   4 bnd_column_kernel  per map and scored class the plane g uint16 [H][W]: the vertical distance to the nearest contour pixel of the
//                        class in the column, BND_FAR without one.  A thread owns one segment of one column of one plane, lanes are
//                        adjacent columns (coalesced); no sweep carries anything from row to row
//   5 bnd_query_kernel   a workgroup owns a tile of BND_TH x BND_TW pixels of one code map, a wave rows of it.  For a contour pixel (y, x)
//                        of class c, best = min over dx of dx^2 + g[y][x +- dx]^2 in the other map's plane c, dx = 0, 1, ... while
//                        dx^2 < best: exact, because a nearest contour pixel in column x' is the nearest one of that column.  Every
//                        lane first widens for its own pixel up to BND_NEAR columns, which settles contours that lie close; the
//                        pixels left over the wave takes one after the other and searches together, lane l at dx = base + l, a wave
//                        minimum, base += 64.  A class the other map has no contour of (present) is not searched for at all.  Count, maximum and histogram gather in an LDS copy of the tile's rows of `out` when nc
//                        (2 + bins) <= BND_LDS_WORDS (LDS = true) and leave as one atomic per non-zero word, else they go out directly
// Integer arithmetic and integer atomics (add, max) only.  No kernel uses scratch memory or waits on another workgroup.
#define BND_TH 16
#define BND_TW 64
#define BND_THREADS 256
#define BND_COLS 64
#define BND_SEG 64
#define BND_NEAR 8
#define BND_LDS_WORDS 8192
#define BND_NONE 255u
#define BND_FAR 65535u
#define BND_INF 0x7fffffff

__global__ __launch_bounds__(BND_THREADS) void bnd_fill_kernel(int* __restrict__ out, long words, int nc, int row, unsigned long long skip,
                                                               unsigned long long* __restrict__ present, int maps) {
  const long i = (long)blockIdx.x * BND_THREADS + threadIdx.x;
  if (i < maps) present[i] = 0ull;                                        // (bnd_mask_kernel gathers into them)
  if (i >= words) return;
  const int j = (int)(i % row), c = (int)((i / (2 * row)) % nc);
  out[i] = (skip >> c & 1ull) ? 0 : j == 1 ? -1 : 0;
}

// the class of value v, BND_NONE for a value outside 0 .. nc-1 or a skipped class
__device__ __forceinline__ unsigned bnd_class(long long v, int nc, unsigned long long skip) {
  return v >= 0 && v < nc && !(skip >> v & 1ull) ? (unsigned)v : BND_NONE;
}

template <typename T>
__device__ __forceinline__ unsigned bnd_code(const T* __restrict__ m, int y, int x, int H, int W, int nc, unsigned long long skip) {
  const T* p = m + (long)y * W + x;
  const T v = *p;
  const unsigned c = bnd_class((long long)v, nc, skip);
  if (c == BND_NONE) return BND_NONE;
  const bool edge = y == 0 || y == H - 1 || x == 0 || x == W - 1 || p[-W] != v || p[W] != v || p[-1] != v || p[1] != v;
  return edge ? c : BND_NONE;
}

__global__ __launch_bounds__(BND_THREADS) void bnd_mark_kernel(const long long* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                               unsigned char* __restrict__ codes, long pixels, int n, int H, int W, int nc,
                                                               unsigned long long skip) {
  const long i = (long)blockIdx.x * BND_THREADS + threadIdx.x;           // (f, y, x)
  if (i >= pixels) return;
  const long hw = (long)H * W;
  const long f = i / hw, r = i - f * hw;
  const int y = (int)(r / W), x = (int)(r - (long)y * W);
  codes[i] = (unsigned char)bnd_code(gt + f * hw, y, x, H, W, nc, skip);
  codes[pixels + i] = (unsigned char)bnd_code(pred + f * hw, y, x, H, W, nc, skip);
}

// bit r of the result: row y0 + r of the column at cm (stride W) holds code c; rows from H on hold nothing.  64 independent loads.
__device__ __forceinline__ unsigned long long bnd_seg_bits(const unsigned char* __restrict__ cm, int y0, int H, int W, unsigned c) {
  unsigned long long m = 0;
#pragma unroll
  for (int r = 0; r < BND_SEG; ++r)
    if (y0 + r < H && cm[(long)(y0 + r) * W] == c) m |= 1ull << r;
  return m;
}

// grid: (map m, frame f, segment s of BND_SEG rows, band of BND_COLS columns), the band fastest: table[m n + f][s][x] = the classes
// that have a contour pixel in the segment's rows of column x, one bit per class; present[m n + f] = the classes of the whole map
__global__ __launch_bounds__(BND_COLS) void bnd_mask_kernel(const unsigned char* __restrict__ codes, unsigned long long* __restrict__ table,
                                                            unsigned long long* present, int H, int W, int S, int bands) {
  unsigned b = blockIdx.x;
  const int band = (int)(b % (unsigned)bands);
  b /= (unsigned)bands;
  const int s = (int)(b % (unsigned)S);
  const long mf = (long)(b / (unsigned)S);
  const int x = band * BND_COLS + (int)threadIdx.x;
  const unsigned char* cm = codes + mf * H * W + x;
  unsigned long long m = 0;
  if (x < W) {
#pragma unroll 16
    for (int r = 0; r < BND_SEG; ++r) {
      const int y = s * BND_SEG + r;
      const unsigned code = y < H ? cm[(long)y * W] : BND_NONE;
      if (code != BND_NONE) m |= 1ull << code;
    }
    table[(mf * S + s) * W + x] = m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o);                 // the workgroup is one wave: its classes, then the map's
  if (threadIdx.x == 0 && m) atomicOr(present + mf, m);
}

// grid: (map m, frame f, class c, segment s, band of BND_COLS columns), the band fastest.  A thread owns BND_SEG rows of one column of
// one plane: its own rows' contour pixels of the class as a bit mask, the nearest one above and below the segment through the table
// (the first segment in that direction whose bit c is set, then that segment's rows), and every row's distance from bit counts.
__global__ __launch_bounds__(BND_COLS) void bnd_column_kernel(const unsigned char* __restrict__ codes, const unsigned long long* __restrict__ table,
                                                              unsigned short* __restrict__ g, int H, int W, int nc, int S, int bands,
                                                              unsigned long long skip) {
  unsigned b = blockIdx.x;
  const int band = (int)(b % (unsigned)bands);
  b /= (unsigned)bands;
  const int s = (int)(b % (unsigned)S);
  b /= (unsigned)S;
  const int c = (int)(b % (unsigned)nc);
  const long mf = (long)(b / (unsigned)nc);                               // m n + f
  const int x = band * BND_COLS + (int)threadIdx.x;
  if ((skip >> c & 1ull) || x >= W) return;                               // (a skipped class has no contour pixel: nobody reads its plane)
  const unsigned char* cm = codes + mf * H * W + x;
  const unsigned long long* tb = table + mf * S * W + x;
  unsigned short* gp = g + (mf * nc + c) * (long)H * W + x;
  const int y0 = s * BND_SEG;
  const unsigned long long own = (tb[(long)s * W] >> c & 1ull) ? bnd_seg_bits(cm, y0, H, W, (unsigned)c) : 0ull;
  int above = -1, below = -1;                                             // the nearest contour row outside the segment, -1: none
  for (int t = s - 1; t >= 0; --t)
    if (tb[(long)t * W] >> c & 1ull) {
      above = t * BND_SEG + 63 - __clzll((long long)bnd_seg_bits(cm, t * BND_SEG, H, W, (unsigned)c));
      break;
    }
  for (int t = s + 1; t < S; ++t)
    if (tb[(long)t * W] >> c & 1ull) {
      below = t * BND_SEG + __ffsll((long long)bnd_seg_bits(cm, t * BND_SEG, H, W, (unsigned)c)) - 1;
      break;
    }
#pragma unroll 8
  for (int r = 0; r < BND_SEG; ++r) {
    const int y = y0 + r;
    if (y >= H) break;
    const unsigned long long lo = own & (~0ull >> (63 - r)), hi = own >> r;     // the segment's contour rows <= y, and >= y from bit 0
    const unsigned up = lo ? (unsigned)(r - (63 - __clzll((long long)lo))) : above >= 0 ? (unsigned)(y - above) : BND_FAR;
    const unsigned down = hi ? (unsigned)(__ffsll((long long)hi) - 1) : below >= 0 ? (unsigned)(below - y) : BND_FAR;
    gp[(long)y * W] = (unsigned short)min(up, down);
  }
}

// the smallest k with k k >= d2 (d2 < 2^30): the float root seeds, integer comparisons decide
__device__ __forceinline__ int bnd_ceil_sqrt(int d2) {
  int k = (int)sqrtf((float)d2);
  while (k > 0 && (k - 1) * (k - 1) >= d2) --k;
  while (k * k < d2) ++k;
  return k;
}

// grid: (map m, frame f, tile row, tile column), the tile column fastest; m is the direction d of the rows it adds to
template <bool LDS>
__global__ __launch_bounds__(BND_THREADS) void bnd_query_kernel(const unsigned char* __restrict__ codes, const unsigned short* __restrict__ g,
                                                                const unsigned long long* __restrict__ present, int* out, int n, int H,
                                                                int W, int nc, int bins, int tx, int ty) {
  __shared__ int tab[LDS ? BND_LDS_WORDS : 1];
  const int row = 2 + bins;
  unsigned b = blockIdx.x;
  const int bx = (int)(b % (unsigned)tx);
  b /= (unsigned)tx;
  const int by = (int)(b % (unsigned)ty);
  b /= (unsigned)ty;
  const int f = (int)(b % (unsigned)n), m = (int)(b / (unsigned)n);
  if (LDS) {
    for (int i = (int)threadIdx.x; i < nc * row; i += BND_THREADS) tab[i] = i % row == 1 ? -1 : 0;
    __syncthreads();
  }
  const long hw = (long)H * W;
  const unsigned char* cm = codes + ((long)m * n + f) * hw;
  const unsigned short* other = g + ((long)(1 - m) * n + f) * nc * hw;
  int* of = out + ((long)f * nc * 2 + m) * row;                           // class c's row of this direction: of + 2 c row
  const unsigned long long there = present[(long)(1 - m) * n + f];       // the classes the other map has a contour of
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;   // BND_TW is the wave's width: a wave owns rows of the tile
  const int x = bx * BND_TW + lane;
  for (int yy = wave; yy < BND_TH; yy += BND_THREADS / 64) {
    const int y = by * BND_TH + yy;
    if (y >= H) break;                                                    // (the whole wave)
    const unsigned code = x < W ? cm[(long)y * W + x] : BND_NONE;
    // every lane searches for its own pixel up to BND_NEAR columns to both sides; that settles the pixel when best <= (BND_NEAR + 1)^2
    int mine = BND_INF;
    bool far = false;
    if (code != BND_NONE && (there >> code & 1ull)) {
      const unsigned short* gr = other + (long)code * hw + (long)y * W;
      const int g0 = gr[x];
      if (g0 != (int)BND_FAR) mine = g0 * g0;
      int dx = 1;
      for (; dx <= BND_NEAR && dx * dx < mine; ++dx) {
        const int l = x - dx >= 0 ? (int)gr[x - dx] : (int)BND_FAR, r = x + dx < W ? (int)gr[x + dx] : (int)BND_FAR;
        const int v = min(l, r);
        if (v != (int)BND_FAR) mine = min(mine, dx * dx + v * v);
      }
      far = dx * dx < mine && (x - dx >= 0 || x + dx < W);               // columns from dx on could still be nearer
    }
    unsigned long long todo = __ballot(far);
    while (todo) {                                                        // the others one after the other, the wave searches together
      const int i = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const unsigned c = (unsigned)__shfl((int)code, i);
      const int xp = bx * BND_TW + i;
      const unsigned short* gr = other + (long)c * hw + (long)y * W;
      int best = __shfl(mine, i);
      for (int base = BND_NEAR + 1;; base += 64) {                        // lane l takes the columns xp - dx and xp + dx, dx = base + l
        const int dx = base + lane;
        const int l = xp - dx >= 0 ? (int)gr[xp - dx] : (int)BND_FAR, r = xp + dx < W ? (int)gr[xp + dx] : (int)BND_FAR;
        const int v = min(l, r);
        int cand = v == (int)BND_FAR ? BND_INF : dx * dx + v * v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
        best = min(best, cand);
        const int nb = base + 64;                                         // every column further out has dx >= nb
        if (nb * nb >= best || (xp - nb < 0 && xp + nb >= W)) break;
      }
      if (lane == i) mine = best;
    }
    if (code != BND_NONE) {
      int* t = LDS ? tab + (int)code * row : of + 2 * (long)code * row;
      atomicAdd(t, 1);
      if (mine != BND_INF) {
        atomicMax(t + 1, mine);
        atomicAdd(t + 2 + min(bnd_ceil_sqrt(mine), bins - 1), 1);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nc * row; i += BND_THREADS) {
      const int v = tab[i], c = i / row, j = i - c * row;
      if (j == 1) {
        if (v >= 0) atomicMax(of + 2 * (long)c * row + 1, v);
      } else if (v != 0) {
        atomicAdd(of + 2 * (long)c * row + j, v);
      }
    }
  }
}

extern "C" int stswin_boundary_geometry(int which) {
  return which == 0 ? BND_TH : which == 1 ? BND_TW : which == 2 ? BND_COLS : which == 3 ? BND_SEG : -1;
}

extern "C" long stswin_boundary_scratch(int n, int H, int W, int nc) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1870;
  if (nc < 1 || nc > 64) return -1872;
  const long S = (H + BND_SEG - 1) / BND_SEG;
  // the table uint64 [2][n][S][W], the maps' classes uint64 [2][n], the planes uint16 [2][n][nc][H][W], the codes uint8 [2][n][H][W]
  return 16 * (long)n * (S * W + 1) + 2 * (long)n * H * W * (2 * (long)nc + 1);
}

extern "C" int stswin_boundary_counts(const long long* gt, const unsigned char* pred, int* out, int n, int H, int W, int nc, int bins,
                                      long skip_mask, void* workspace, long workspace_bytes, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1870;
  if (gt == nullptr || pred == nullptr || out == nullptr || workspace == nullptr) return -1871;
  if (nc < 1 || nc > 64) return -1872;
  if (bins < 2 || bins > 256) return -1873;
  if (workspace_bytes < stswin_boundary_scratch(n, H, W, nc) || ((uintptr_t)workspace & 7)) return -1874;
  if (((uintptr_t)gt & 7) || ((uintptr_t)out & 3)) return -1875;
  const long pixels = (long)n * H * W, words = (long)n * nc * 2 * (2 + bins);
  const int bands = (W + BND_COLS - 1) / BND_COLS, tx = (W + BND_TW - 1) / BND_TW, ty = (H + BND_TH - 1) / BND_TH;
  const long fill_blocks = (words + BND_THREADS - 1) / BND_THREADS, mark_blocks = (pixels + BND_THREADS - 1) / BND_THREADS;
  const int S = (H + BND_SEG - 1) / BND_SEG;
  const long mask_blocks = 2 * (long)n * S * bands, col_blocks = mask_blocks * nc, query_blocks = 2 * (long)n * tx * ty;
  if (fill_blocks > 0x7fffffffL || mark_blocks > 0x7fffffffL || col_blocks > 0x7fffffffL || query_blocks > 0x7fffffffL) return -1870;
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long skip = (unsigned long long)skip_mask;
  unsigned long long* table = reinterpret_cast<unsigned long long*>(workspace);
  unsigned long long* present = table + 2 * (long)n * S * W;
  unsigned short* g = reinterpret_cast<unsigned short*>(present + 2 * n);
  unsigned char* codes = reinterpret_cast<unsigned char*>(g) + 4 * pixels * nc;
  hipLaunchKernelGGL(bnd_fill_kernel, dim3((unsigned)fill_blocks), dim3(BND_THREADS), 0, st, out, words, nc, 2 + bins, skip, present, 2 * n);
  hipLaunchKernelGGL(bnd_mark_kernel, dim3((unsigned)mark_blocks), dim3(BND_THREADS), 0, st, gt, pred, codes, pixels, n, H, W, nc, skip);
  hipLaunchKernelGGL(bnd_mask_kernel, dim3((unsigned)mask_blocks), dim3(BND_COLS), 0, st, (const unsigned char*)codes, table, present, H, W, S, bands);
  hipLaunchKernelGGL(bnd_column_kernel, dim3((unsigned)col_blocks), dim3(BND_COLS), 0, st, (const unsigned char*)codes,
                     (const unsigned long long*)table, g, H, W, nc, S, bands, skip);
  if (nc * (2 + bins) <= BND_LDS_WORDS)
    hipLaunchKernelGGL(bnd_query_kernel<true>, dim3((unsigned)query_blocks), dim3(BND_THREADS), 0, st, (const unsigned char*)codes,
                       (const unsigned short*)g, (const unsigned long long*)present, out, n, H, W, nc, bins, tx, ty);
  else
    hipLaunchKernelGGL(bnd_query_kernel<false>, dim3((unsigned)query_blocks), dim3(BND_THREADS), 0, st, (const unsigned char*)codes,
                       (const unsigned short*)g, (const unsigned long long*)present, out, n, H, W, nc, bins, tx, ty);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Clearance of the instances (stswincl_amd/utils/instruments.py, instance_clearance, states the result; VideoSegmenter(clearance=...)):
// per instance ordinal i < K and target class c that the instance does not hold itself, the smallest squared Euclidean distance d2
// between a pixel p of the instance and a pixel q of the class, with the first such p and, for it, the first such q in raster order.
// Six launches whatever nc, K and the maps hold, the two in the middle being the boundary scores' own, over n maps instead of 2 n:
//   1 clr_fill_kernel     keys uint64 [n][K][nc] all ones (no pair yet), own uint64 [n][K] and present uint64 [n] zero
//   2 clr_mark_kernel     labels -> the code map uint8 [n][H][W] (bnd_code: the pixel's class where it is a contour pixel of a target
//                         class, BND_NONE elsewhere) and own[f][i], the classes instance i holds, one bit each.  The bit is set from
//                         the first pixel of every horizontal run of equal (ordinal, class) - every class an instance holds starts
//                         such a run, whatever the ordinals have to do with the labels - and only where it is not set yet
//   3 bnd_mask_kernel, 4 bnd_column_kernel   as they stand: the planes g uint16 [n][nc][H][W] of the target classes
//   5 clr_query_kernel    bnd_query_kernel's tiling.  A pixel p of ordinal i in 0 .. K-1 takes part when a 4-neighbour has another
//                         ordinal or lies outside the image.  That loses nothing: were all four neighbours of a minimising p in the
//                         instance, the one a step towards q (along the axis of the larger |p - q| component; q != p because the
//                         instance holds no pixel of the class) would be of the instance and strictly nearer to q.  The same step
//                         taken from q shows that the nearest pixel of the class is a contour pixel of it, so the planes, which hold
//                         the contours only, give every p outside the class its exact distance to the class.  Per present target
//                         class c outside own[f][i] the search of bnd_query_kernel runs under the bound min(d2 of the current key,
//                         max_d2) + 1 - a distance equal to the key's still counts, its p may be the smaller one; a stale, larger
//                         key only costs columns - and what it finds below the bound goes into the key d2 << 28 | p by a 64-bit
//                         atomicMin (d2 < 2^30, p < 2^28): the smallest d2, and among its pixels the smallest p, in any order.
//                         Where the near search leaves more than CLR_SOLO pixels of a row over (a horizontal stretch of border far
//                         from the class), the row searches at once instead of pixel by pixel: the same minimum, each column
//                         loaded once for all of them and dropped for all when its g^2 cannot lower the worst of them
//   6 clr_resolve_kernel  a wave per (f, i, c): no key -> three -1; else over the rows y + dy, |dy| <= floor(sqrt(d2)), with d2 - dy^2
//                         a perfect square dx^2, the pixels (y + dy, x -+ dx) with labels == c, the smallest index by a wave minimum
// Integer arithmetic and integer atomics (or, min) only; the float root only seeds the integer root, comparisons decide it.  No kernel
// uses scratch memory or waits on another workgroup.
#define CLR_P_BITS 28
#define CLR_NO_KEY (~0ull)
#define CLR_SOLO 2                      // up to that many pixels of a row left over by the near search are searched for one by one

__global__ __launch_bounds__(BND_THREADS) void clr_fill_kernel(unsigned long long* __restrict__ keys, long nkeys,
                                                               unsigned long long* __restrict__ own, long nown,
                                                               unsigned long long* __restrict__ present, int maps) {
  const long i = (long)blockIdx.x * BND_THREADS + threadIdx.x;
  if (i < maps) present[i] = 0ull;                                        // (bnd_mask_kernel gathers into them)
  if (i < nown) own[i] = 0ull;
  if (i < nkeys) keys[i] = CLR_NO_KEY;
}

__global__ __launch_bounds__(BND_THREADS) void clr_mark_kernel(const unsigned char* __restrict__ labels, const int* __restrict__ comp,
                                                               unsigned char* __restrict__ codes, unsigned long long* own, long pixels,
                                                               int H, int W, int nc, int K, unsigned long long skip) {
  const long i = (long)blockIdx.x * BND_THREADS + threadIdx.x;           // (f, y, x)
  if (i >= pixels) return;
  const long hw = (long)H * W;
  const long f = i / hw, r = i - f * hw;
  const int y = (int)(r / W), x = (int)(r - (long)y * W);
  codes[i] = (unsigned char)bnd_code(labels + f * hw, y, x, H, W, nc, skip);
  const int o = comp[i];
  const unsigned v = labels[i];
  if (o < 0 || o >= K || v >= (unsigned)nc) return;
  if (x > 0 && comp[i - 1] == o && labels[i - 1] == v) return;            // not the first pixel of its run
  unsigned long long* w = own + f * K + o;
  if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> v & 1ull)) atomicOr(w, 1ull << v);
}

// grid: (frame f, tile row, tile column), the tile column fastest
__global__ __launch_bounds__(BND_THREADS) void clr_query_kernel(const int* __restrict__ comp, const unsigned short* __restrict__ g,
                                                                const unsigned long long* __restrict__ present,
                                                                const unsigned long long* __restrict__ own, unsigned long long* keys,
                                                                int H, int W, int nc, int K, unsigned long long targets, int limit,
                                                                int tx, int ty) {
  unsigned b = blockIdx.x;
  const int bx = (int)(b % (unsigned)tx);
  b /= (unsigned)tx;
  const int by = (int)(b % (unsigned)ty);
  const long f = (long)(b / (unsigned)ty);
  const unsigned long long there = present[f] & targets;                  // the target classes the map has a pixel of
  if (!there) return;
  const long hw = (long)H * W;
  const int* cf = comp + f * hw;
  const unsigned short* planes = g + f * nc * hw;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;   // BND_TW is the wave's width: a wave owns rows of the tile
  const int x = bx * BND_TW + lane;
  for (int yy = wave; yy < BND_TH; yy += BND_THREADS / 64) {
    const int y = by * BND_TH + yy;
    if (y >= H) break;                                                    // (the whole wave)
    int ord = -1;                                                         // the ordinal of a pixel that takes part, else -1
    if (x < W) {
      const int* p = cf + (long)y * W + x;
      const int o = *p;
      if (o >= 0 && o < K &&
          (y == 0 || y == H - 1 || x == 0 || x == W - 1 || p[-W] != o || p[W] != o || p[-1] != o || p[1] != o))
        ord = o;
    }
    if (!__ballot(ord >= 0)) continue;
    const unsigned long long held = ord >= 0 ? own[f * K + ord] : ~0ull;
    unsigned long long* kp = keys + (f * K + max(ord, 0)) * nc;
    const unsigned long long at = (unsigned long long)((long)y * W + x);
    for (unsigned long long cs = there; cs; cs &= cs - 1) {
      const int c = __ffsll((long long)cs) - 1;
      const bool take = ord >= 0 && !(held >> c & 1ull);
      if (!__ballot(take)) continue;
      const unsigned short* gr = planes + (long)c * hw + (long)y * W;
      // every lane searches for its own pixel up to BND_NEAR columns to both sides; that settles the pixel when best <= (BND_NEAR + 1)^2
      int bound = 0, mine = 0;
      bool far = false;
      if (take) {
        const unsigned long long d = __hip_atomic_load(kp + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> CLR_P_BITS;
        bound = (d < (unsigned long long)limit ? (int)d : limit) + 1;     // only a d2 < bound is of interest
        mine = bound;
        const int g0 = gr[x];
        if (g0 != (int)BND_FAR) mine = min(mine, g0 * g0);
        int dx = 1;
        for (; dx <= BND_NEAR && dx * dx < mine; ++dx) {
          const int l = x - dx >= 0 ? (int)gr[x - dx] : (int)BND_FAR, r = x + dx < W ? (int)gr[x + dx] : (int)BND_FAR;
          const int v = min(l, r);
          if (v != (int)BND_FAR) mine = min(mine, dx * dx + v * v);
        }
        far = dx * dx < mine && (x - dx >= 0 || x + dx < W);             // columns from dx on could still be nearer
      }
      unsigned long long todo = __ballot(far);
      if (__popcll(todo) > CLR_SOLO) {
        // many of the row's pixels are left over: the row searches at once.  Ring k is the 64 columns of the tile (k = 0) or the 64
        // columns 64 k to the left and to the right of them; a lane loads one column of the ring, and every column that can still
        // matter to the worst lane (g^2 below the largest best among the lanes left over) is handed to all lanes, one readlane each
        int bmax = far ? mine : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bmax = max(bmax, __shfl_xor(bmax, o));
        const int x0 = bx * BND_TW;
        for (int k = 0;; ++k) {
          const int reach = 64 * k - 63;                                  // the smallest |dx| between a lane and a column of ring k >= 1
          if (k > 0 && (reach * reach >= bmax || (x0 - reach < 0 && x0 + 64 * k >= W))) break;
          for (int side = 0; side < (k == 0 ? 1 : 2); ++side) {
            const int cs = side == 0 ? x0 - 64 * k : x0 + 64 * k;
            const int xc = cs + lane;
            const int v = xc >= 0 && xc < W ? (int)gr[xc] : (int)BND_FAR;
            const int v2 = v == (int)BND_FAR ? BND_INF : v * v;
            unsigned long long m = __ballot(v2 < bmax);
            while (m) {
              const int j = __ffsll((long long)m) - 1;
              m &= m - 1;
              const int dx = x - (cs + j);
              mine = min(mine, __mul24(dx, dx) + __builtin_amdgcn_readlane(v2, j));
            }
          }
          bmax = far ? mine : 0;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) bmax = max(bmax, __shfl_xor(bmax, o));
        }
        todo = 0;
      }
      while (todo) {                                                      // few: one after the other, the wave searches together
        const int i = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int xp = bx * BND_TW + i;
        int best = __shfl(mine, i);
        for (int base = BND_NEAR + 1;; base += 64) {                      // lane l takes the columns xp - dx and xp + dx, dx = base + l
          const int dx = base + lane;
          const int l = xp - dx >= 0 ? (int)gr[xp - dx] : (int)BND_FAR, r = xp + dx < W ? (int)gr[xp + dx] : (int)BND_FAR;
          const int v = min(l, r);
          int cand = v == (int)BND_FAR ? BND_INF : dx * dx + v * v;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
          best = min(best, cand);
          const int nb = base + 64;                                       // every column further out has dx >= nb
          if (nb * nb >= best || (xp - nb < 0 && xp + nb >= W)) break;
        }
        if (lane == i) mine = best;
      }
      if (take && mine < bound) atomicMin(kp + c, (unsigned long long)mine << CLR_P_BITS | at);
    }
  }
}

// the largest k with k k <= d2 (d2 < 2^30): the float root seeds, integer comparisons decide
__device__ __forceinline__ int clr_floor_sqrt(int d2) {
  int k = (int)sqrtf((float)d2);
  while (k * k > d2) --k;
  while ((k + 1) * (k + 1) <= d2) ++k;
  return k;
}

// a wave per entry e = (f, i, c) of the keys; a workgroup takes BND_THREADS / 64 of them
__global__ __launch_bounds__(BND_THREADS) void clr_resolve_kernel(const unsigned char* __restrict__ labels,
                                                                  const unsigned long long* __restrict__ keys,
                                                                  long long* __restrict__ out, long entries, int H, int W, int nc, int K) {
  const long e = (long)blockIdx.x * (BND_THREADS / 64) + (threadIdx.x >> 6);
  if (e >= entries) return;                                               // (the whole wave)
  const int lane = (int)threadIdx.x & 63;
  const unsigned long long key = keys[e];
  long long* o = out + 3 * e;
  if (key == CLR_NO_KEY) {
    if (lane < 3) o[lane] = -1;
    return;
  }
  const unsigned c = (unsigned)(e % nc);
  const unsigned char* lab = labels + e / ((long)K * nc) * H * W;
  const int d2 = (int)(key >> CLR_P_BITS), p = (int)(key & ((1ull << CLR_P_BITS) - 1));
  const int y = p / W, x = p - y * W;
  const int R = clr_floor_sqrt(d2);
  int q = BND_INF;
  for (int t = lane; t <= 2 * R; t += 64) {
    const int dy = t - R, yq = y + dy;
    if (yq < 0 || yq >= H) continue;
    const int rem = d2 - dy * dy, dx = clr_floor_sqrt(rem);
    if (dx * dx != rem) continue;
    const unsigned char* row = lab + (long)yq * W;
    if (x + dx < W && row[x + dx] == c) q = min(q, yq * W + x + dx);
    if (x - dx >= 0 && row[x - dx] == c) q = min(q, yq * W + x - dx);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) q = min(q, __shfl_xor(q, s));
  if (lane == 0) {
    o[0] = d2;
    o[1] = p;
    o[2] = q;
  }
}

extern "C" int stswin_instance_clearance_geometry(int which) {
  return which == 4 ? BND_NEAR : which == 5 ? CLR_SOLO : stswin_boundary_geometry(which);
}

extern "C" long stswin_instance_clearance_scratch(int n, int H, int W, int nc, int K) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1920;
  if (nc < 1 || nc > 64) return -1922;
  if (K < 1 || K > 1024) return -1923;
  const long S = (H + BND_SEG - 1) / BND_SEG;
  // the table uint64 [n][S][W], the maps' classes uint64 [n], the keys uint64 [n][K][nc], the instances' classes uint64 [n][K], the
  // planes uint16 [n][nc][H][W], the codes uint8 [n][H][W]
  return 8 * (long)n * (S * W + 1 + (long)K * nc + K) + (long)n * H * W * (2 * (long)nc + 1);
}

extern "C" int stswin_instance_clearance(const unsigned char* labels, const int* components, long long* out, int n, int H, int W, int nc,
                                         int K, long target_mask, long max_d2, void* workspace, long workspace_bytes, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384) return -1920;
  if (labels == nullptr || components == nullptr || out == nullptr || workspace == nullptr) return -1921;
  if (nc < 1 || nc > 64) return -1922;
  if (K < 1 || K > 1024) return -1923;
  if (workspace_bytes < stswin_instance_clearance_scratch(n, H, W, nc, K) || ((uintptr_t)workspace & 7)) return -1924;
  if (((uintptr_t)components & 3) || ((uintptr_t)out & 7)) return -1925;
  if (max_d2 < -1) return -1926;
  const long pixels = (long)n * H * W, nkeys = (long)n * K * nc, nown = (long)n * K;
  const int bands = (W + BND_COLS - 1) / BND_COLS, tx = (W + BND_TW - 1) / BND_TW, ty = (H + BND_TH - 1) / BND_TH;
  const int S = (H + BND_SEG - 1) / BND_SEG;
  const long fill_blocks = (nkeys + BND_THREADS - 1) / BND_THREADS, mark_blocks = (pixels + BND_THREADS - 1) / BND_THREADS;
  const long mask_blocks = (long)n * S * bands, col_blocks = mask_blocks * nc, query_blocks = (long)n * tx * ty;
  const long resolve_blocks = (nkeys + BND_THREADS / 64 - 1) / (BND_THREADS / 64);
  if (fill_blocks > 0x7fffffffL || mark_blocks > 0x7fffffffL || col_blocks > 0x7fffffffL || query_blocks > 0x7fffffffL ||
      resolve_blocks > 0x7fffffffL)
    return -1920;
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long all = nc == 64 ? ~0ull : (1ull << nc) - 1;
  const unsigned long long targets = (unsigned long long)target_mask & all;
  const int limit = max_d2 < 0 || max_d2 > (1L << 30) ? 1 << 30 : (int)max_d2;            // every d2 is < 2^30
  unsigned long long* table = reinterpret_cast<unsigned long long*>(workspace);
  unsigned long long* present = table + (long)n * S * W;
  unsigned long long* keys = present + n;
  unsigned long long* own = keys + nkeys;
  unsigned short* g = reinterpret_cast<unsigned short*>(own + nown);
  unsigned char* codes = reinterpret_cast<unsigned char*>(g) + 2 * pixels * nc;
  hipLaunchKernelGGL(clr_fill_kernel, dim3((unsigned)fill_blocks), dim3(BND_THREADS), 0, st, keys, nkeys, own, nown, present, n);
  hipLaunchKernelGGL(clr_mark_kernel, dim3((unsigned)mark_blocks), dim3(BND_THREADS), 0, st, labels, components, codes, own, pixels, H, W,
                     nc, K, ~targets);
  hipLaunchKernelGGL(bnd_mask_kernel, dim3((unsigned)mask_blocks), dim3(BND_COLS), 0, st, (const unsigned char*)codes, table, present, H, W, S, bands);
  hipLaunchKernelGGL(bnd_column_kernel, dim3((unsigned)col_blocks), dim3(BND_COLS), 0, st, (const unsigned char*)codes,
                     (const unsigned long long*)table, g, H, W, nc, S, bands, ~targets);
  hipLaunchKernelGGL(clr_query_kernel, dim3((unsigned)query_blocks), dim3(BND_THREADS), 0, st, components, (const unsigned short*)g,
                     (const unsigned long long*)present, (const unsigned long long*)own, keys, H, W, nc, K, targets, limit, tx, ty);
  hipLaunchKernelGGL(clr_resolve_kernel, dim3((unsigned)resolve_blocks), dim3(BND_THREADS), 0, st, labels,
                     (const unsigned long long*)keys, out, nkeys, H, W, nc, K);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Frames as a video source delivers them (stswincl_amd/utils/yuv.py states the arithmetic): NV12 or UYVY -> the HWC RGB frame that
// stswin_frame_ingest and stswin_labels_overlay read, and RGB -> NV12.  matrix int32 [3][4]: out_c = clamp((m[c][0] t0 + m[c][1] t1 +
// m[c][2] t2 + m[c][3]) >> 14, 0, 255) in int32 (|sum| < 2^25).  A thread owns YUV_PPT = 8 (wide body) or 2 (byte body) consecutive
// pixels of one row, and for NV12 of the two luma rows that share a chroma row, so each (U, V) pair is fetched once: NV12 wide reads
// two 8-byte luma runs and one 8-byte chroma run (linear: the rows above and below too, and one pair to the right as two bytes), UYVY
// wide one 16-byte run; each RGB row of 24 bytes leaves as three 8-byte stores.  The wide body needs Ws % 8 == 0 (then every row and
// every frame starts on the grid) and the pointers 8-byte (UYVY in: 16-byte) aligned; anything else takes the byte body.  Threads are
// numbered (frame, row pair | row, group) with the group fastest: consecutive lanes read and write consecutive runs.
#define YUV_PPT 8

__device__ __forceinline__ unsigned yuv_channel(const int* m, int c, int t0, int t1, int t2) {
  // clamp, then shift: the same value as clamp(v >> 14, 0, 255), the shift being monotonic.  Written the other way round the compiler
  // packs two results with v_ashr_pk_u8_i32, which writes 16 bits, and ORs a third byte into the stale upper half of that register
  const int v = m[4 * c] * t0 + m[4 * c + 1] * t1 + m[4 * c + 2] * t2 + m[4 * c + 3];
  return (unsigned)(min(max(v, 0), (256 << 14) - 1) >> 14);
}

// NP (U, V) pairs from k0 on, and for LINEAR the pair kn to their right (already clamped to the row), of one NV12 chroma row
template <bool WIDE, bool LINEAR, int NP>
__device__ __forceinline__ void nv12_pairs(const unsigned char* row, int k0, int kn, int* u, int* v) {
  if (WIDE) {
    const uint2 w = *reinterpret_cast<const uint2*>(row + 2 * k0);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const unsigned d = (i < 2 ? w.x : w.y) >> (16 * (i & 1));
      u[i] = (int)(d & 255u);
      v[i] = (int)((d >> 8) & 255u);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      u[i] = row[2 * (k0 + i)];
      v[i] = row[2 * (k0 + i) + 1];
    }
  }
  u[NP] = LINEAR ? (int)row[2 * kn] : 0;
  v[NP] = LINEAR ? (int)row[2 * kn + 1] : 0;
}

template <int FMT, bool LINEAR, bool WIDE>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const unsigned char* __restrict__ in, const int* __restrict__ matrix,
                                                         unsigned char* __restrict__ out, unsigned total, int Hs, int Ws) {
  constexpr int PX = WIDE ? YUV_PPT : 2, NP = PX / 2, ROWS = FMT == 0 ? 2 : 1;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  int m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = matrix[i];
  const unsigned G = (unsigned)(Ws / PX), R = (unsigned)(Hs / ROWS);
  const unsigned g = t % G, fj = t / G;
  const int j = (int)(fj % R);
  const long f = (long)(fj / R);
  const int k0 = (int)g * NP, kn = min(k0 + NP, Ws / 2 - 1);
  int y[ROWS][PX], cu[ROWS][NP + 1], cv[ROWS][NP + 1];
  if (FMT == 0) {
    const unsigned char* fr = in + f * ((long)Hs * Ws / 2 * 3);
    const unsigned char* cp = fr + (long)Hs * Ws;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const unsigned char* lp = fr + (long)(2 * j + r) * Ws + (long)g * PX;
      if (WIDE) {
        const uint2 w = *reinterpret_cast<const uint2*>(lp);
#pragma unroll
        for (int i = 0; i < PX; ++i) y[r][i] = (int)(((i < 4 ? w.x : w.y) >> (8 * (i & 3))) & 255u);
      } else {
#pragma unroll
        for (int i = 0; i < PX; ++i) y[r][i] = lp[i];
      }
    }
    int u0[NP + 1], v0[NP + 1];
    nv12_pairs<WIDE, LINEAR, NP>(cp + (long)j * Ws, k0, kn, u0, v0);
    if (LINEAR) {
      int ua[NP + 1], va[NP + 1], ub[NP + 1], vb[NP + 1];
      nv12_pairs<WIDE, true, NP>(cp + (long)max(j - 1, 0) * Ws, k0, kn, ua, va);
      nv12_pairs<WIDE, true, NP>(cp + (long)min(j + 1, (int)R - 1) * Ws, k0, kn, ub, vb);
#pragma unroll
      for (int i = 0; i <= NP; ++i) {
        cu[0][i] = (3 * u0[i] + ua[i] + 2) >> 2;
        cv[0][i] = (3 * v0[i] + va[i] + 2) >> 2;
        cu[ROWS - 1][i] = (3 * u0[i] + ub[i] + 2) >> 2;
        cv[ROWS - 1][i] = (3 * v0[i] + vb[i] + 2) >> 2;
      }
    } else {
#pragma unroll
      for (int i = 0; i <= NP; ++i) {
        cu[0][i] = cu[ROWS - 1][i] = u0[i];
        cv[0][i] = cv[ROWS - 1][i] = v0[i];
      }
    }
  } else {
    const unsigned char* rp = in + ((f * Hs + j) * Ws) * 2;
    if (WIDE) {
      const uint4 w = *reinterpret_cast<const uint4*>(rp + 4L * k0);
      const unsigned d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        cu[0][i] = (int)(d[i % 4] & 255u);
        y[0][2 * i] = (int)((d[i % 4] >> 8) & 255u);
        cv[0][i] = (int)((d[i % 4] >> 16) & 255u);
        y[0][2 * i + 1] = (int)(d[i % 4] >> 24);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const unsigned char* q = rp + 4L * (k0 + i);
        cu[0][i] = q[0];
        y[0][2 * i] = q[1];
        cv[0][i] = q[2];
        y[0][2 * i + 1] = q[3];
      }
    }
    cu[0][NP] = LINEAR ? (int)rp[4L * kn] : 0;
    cv[0][NP] = LINEAR ? (int)rp[4L * kn + 2] : 0;
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    unsigned o[3 * PX / 4 + 1];
#pragma unroll
    for (int i = 0; i < 3 * PX / 4 + 1; ++i) o[i] = 0u;
    unsigned char* op = out + ((f * Hs + (ROWS * j + r)) * Ws + (long)g * PX) * 3;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const int k = i >> 1;
      const int u = (LINEAR && (i & 1)) ? (cu[r][k] + cu[r][k + 1] + 1) >> 1 : cu[r][k];
      const int v = (LINEAR && (i & 1)) ? (cv[r][k] + cv[r][k + 1] + 1) >> 1 : cv[r][k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned b = yuv_channel(m, c, y[r][i], u, v);
        if (WIDE) o[(3 * i + c) >> 2] |= b << (8 * ((3 * i + c) & 3));
        else op[3 * i + c] = (unsigned char)b;
      }
    }
    if (WIDE) {
      uint2* ow = reinterpret_cast<uint2*>(op);
#pragma unroll
      for (int q = 0; q < 3 * PX / 8; ++q) ow[q] = make_uint2(o[2 * q], o[2 * q + 1]);
    }
  }
}

// RGB -> NV12: a thread owns the PX pixels of both luma rows of a chroma row: luma per pixel through row 0, the 2 x 2 block's
// per-channel mean (sum + 2) >> 2 through rows 1 and 2.  Wide: three 8-byte loads per row, an 8-byte luma store per row, one 8-byte
// chroma store; it needs Ws % 8 == 0 and both pointers 8-byte aligned.
template <bool WIDE>
__global__ __launch_bounds__(256) void rgb_to_nv12_kernel(const unsigned char* __restrict__ in, const int* __restrict__ matrix,
                                                          unsigned char* __restrict__ out, unsigned total, int Hs, int Ws) {
  constexpr int PX = WIDE ? YUV_PPT : 2, NP = PX / 2;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  int m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = matrix[i];
  const unsigned G = (unsigned)(Ws / PX), R = (unsigned)(Hs / 2);
  const unsigned g = t % G, fj = t / G;
  const int j = (int)(fj % R);
  const long f = (long)(fj / R);
  unsigned char* fr = out + f * ((long)Hs * Ws / 2 * 3);
  int sum[NP][3];
#pragma unroll
  for (int k = 0; k < NP; ++k) sum[k][0] = sum[k][1] = sum[k][2] = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const long px = (f * Hs + (2 * j + r)) * Ws + (long)g * PX;
    const unsigned char* ip = in + 3 * px;
    unsigned char* lp = fr + (long)(2 * j + r) * Ws + (long)g * PX;
    unsigned s[3 * PX / 4 + 1];
    if (WIDE) {
      const uint2* iw = reinterpret_cast<const uint2*>(ip);
#pragma unroll
      for (int q = 0; q < 3 * PX / 8; ++q) {
        const uint2 w = iw[q];
        s[2 * q] = w.x;
        s[2 * q + 1] = w.y;
      }
    }
    unsigned yo[PX / 4 + 1];
#pragma unroll
    for (int i = 0; i < PX / 4 + 1; ++i) yo[i] = 0u;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      int c3[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        c3[c] = WIDE ? (int)((s[(3 * i + c) >> 2] >> (8 * ((3 * i + c) & 3))) & 255u) : (int)ip[3 * i + c];
        sum[i >> 1][c] += c3[c];
      }
      const unsigned b = yuv_channel(m, 0, c3[0], c3[1], c3[2]);
      if (WIDE) yo[i >> 2] |= b << (8 * (i & 3));
      else lp[i] = (unsigned char)b;
    }
    if (WIDE) *reinterpret_cast<uint2*>(lp) = make_uint2(yo[0], yo[1 % (PX / 4 + 1)]);
  }
  unsigned char* cp = fr + (long)Hs * Ws + (long)j * Ws + (long)g * PX;
  unsigned co[PX / 4 + 1];
#pragma unroll
  for (int i = 0; i < PX / 4 + 1; ++i) co[i] = 0u;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int r_ = (sum[k][0] + 2) >> 2, g_ = (sum[k][1] + 2) >> 2, b_ = (sum[k][2] + 2) >> 2;
    const unsigned u = yuv_channel(m, 1, r_, g_, b_), v = yuv_channel(m, 2, r_, g_, b_);
    if (WIDE) {
      co[k >> 1] |= (u | (v << 8)) << (16 * (k & 1));
    } else {
      cp[2 * k] = (unsigned char)u;
      cp[2 * k + 1] = (unsigned char)v;
    }
  }
  if (WIDE) *reinterpret_cast<uint2*>(cp) = make_uint2(co[0], co[1 % (PX / 4 + 1)]);
}

static bool yuv_overlap(const void* a, long abytes, const void* b, long bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

extern "C" int stswin_yuv_to_rgb(const unsigned char* in, const int* matrix, unsigned char* out, int n, int Hs, int Ws, int format,
                                 int chroma, void* stream) {
  if (n <= 0 || Hs <= 0 || Ws <= 0) return -1424;
  if (in == nullptr || matrix == nullptr || out == nullptr) return -1425;
  if (format < 0 || format > 1) return -1427;
  if (chroma < 0 || chroma > 1) return -1428;
  if ((Ws & 1) || (format == 0 && (Hs & 1))) return -1426;
  const long px = (long)n * Hs * Ws;
  const long in_bytes = format == 0 ? px / 2 * 3 : px * 2;
  if (yuv_overlap(in, in_bytes, out, 3 * px) || yuv_overlap(matrix, 48, out, 3 * px)) return -1429;
  const bool wide = Ws % YUV_PPT == 0 && (((uintptr_t)in & (format == 0 ? 7 : 15)) | ((uintptr_t)out & 7)) == 0;
  const long threads = px / (format == 0 ? 2 : 1) / (wide ? YUV_PPT : 2);
  const long blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffL) return -1424;                          // (every thread number fits 32 bits)
  dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
#define YUV_LAUNCH(FMT_, LIN_)                                                                                                 \
  do {                                                                                                                         \
    if (wide) hipLaunchKernelGGL((yuv_to_rgb_kernel<FMT_, LIN_, true>), grid, dim3(256), 0, st, in, matrix, out, (unsigned)threads, Hs, Ws); \
    else hipLaunchKernelGGL((yuv_to_rgb_kernel<FMT_, LIN_, false>), grid, dim3(256), 0, st, in, matrix, out, (unsigned)threads, Hs, Ws);    \
  } while (0)
  if (format == 0) {
    if (chroma) YUV_LAUNCH(0, true);
    else YUV_LAUNCH(0, false);
  } else {
    if (chroma) YUV_LAUNCH(1, true);
    else YUV_LAUNCH(1, false);
  }
#undef YUV_LAUNCH
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_rgb_to_nv12(const unsigned char* in, const int* matrix, unsigned char* out, int n, int Hs, int Ws, void* stream) {
  if (n <= 0 || Hs <= 0 || Ws <= 0) return -1424;
  if (in == nullptr || matrix == nullptr || out == nullptr) return -1425;
  if ((Ws & 1) || (Hs & 1)) return -1426;
  const long px = (long)n * Hs * Ws;
  if (yuv_overlap(in, 3 * px, out, px / 2 * 3) || yuv_overlap(matrix, 48, out, px / 2 * 3)) return -1429;
  const bool wide = Ws % YUV_PPT == 0 && (((uintptr_t)in | (uintptr_t)out) & 7) == 0;
  const long threads = px / 2 / (wide ? YUV_PPT : 2);
  const long blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffL) return -1424;
  dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  if (wide) hipLaunchKernelGGL(rgb_to_nv12_kernel<true>, grid, dim3(256), 0, st, in, matrix, out, (unsigned)threads, Hs, Ws);
  else hipLaunchKernelGGL(rgb_to_nv12_kernel<false>, grid, dim3(256), 0, st, in, matrix, out, (unsigned)threads, Hs, Ws);
  STSWIN_CHECK_LAUNCH();
  return 0;
}


// ----------------------------------------------------------------------------------------- statistics from a GEMM epilogue
// A convolution GEMM launched with STSWIN_GF_CS_PARTIAL | STSWIN_GF_CS_SQ leaves per-128-row-block column sums and sums of
// squares of its output in a table [2 planes][nb = 2*ceil(M/256)][N]; this folds the blocks of every BatchNorm statistic group
// (contiguous groups, or interleaved units of unit_rows rows: group = unit index % G) into sum / sumsq [G][N] for
// stswin_bn_finalize (x = NULL: no pivot) - the colstats pass over the activation (one of the three HBM passes of a train-mode
// BatchNorm forward) disappears.  Grid (N / 64, G); 256 threads = 64 columns x 4 block lanes.
__global__ __launch_bounds__(256) void cs_group_reduce_kernel(const float* tab, int nb, int N, int G, int group_rows, int unit,
                                                               float* sum, float* sumsq) {
  __shared__ float red[2][4][64];
  const int cl = threadIdx.x & 63, bl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, g = blockIdx.y;
  float a = 0.f, b = 0.f;
  if (c < N) {
    const float* t1 = tab + c;
    const float* t2 = tab + (long)nb * N + c;
    if (unit <= 0) {
      const int b0 = (int)((long)g * group_rows / 128), b1 = (int)((long)(g + 1) * group_rows / 128);
      for (int k = b0 + bl; k < b1; k += 4) { a += t1[(long)k * N]; b += t2[(long)k * N]; }
    } else {
      const int bpu = unit / 128, units = (int)((long)G * group_rows / unit);
      for (int u = g; u < units; u += G)
        for (int k = u * bpu + bl; k < (u + 1) * bpu; k += 4) { a += t1[(long)k * N]; b += t2[(long)k * N]; }
    }
  }
  red[0][bl][cl] = a;
  red[1][bl][cl] = b;
  __syncthreads();
  if (bl == 0 && c < N) {
    sum[(long)g * N + c] = red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl];
    sumsq[(long)g * N + c] = red[1][0][cl] + red[1][1][cl] + red[1][2][cl] + red[1][3][cl];
  }
}

// BatchNorm statistics straight from a gemm_nt GF_CS_SQ table: group sums over the 128-row blocks, mean / rstd and the
// sequential running-statistic updates (group 0, 1, ... as the per-frame calls of base18.py:86-89 would make them) in ONE
// launch.  1024 threads = 16 columns x 64 block lanes (a 262144-row output has 2048 table rows: 32 independent loads per
// lane and plane); final combination in double.
// PER_GROUP (many groups: the 24 of the batched key views): one workgroup per (16 columns, group) - blockIdx.y = group - writes
// mean / rstd only; bn_running_update_kernel then applies the running-statistic updates in group order.
template <bool PER_GROUP>
__global__ __launch_bounds__(1024) void bn_table_finalize_kernel(const float* tab, int nb, int N, int G, int group_rows, int unit,
                                                                 float* mean, float* rstd, float* running_mean, float* running_var,
                                                                 float eps, float momentum) {
  extern __shared__ float red[];                       // [G][2][16 waves][16 columns]   (PER_GROUP: [1][2][16][16])
  const int cl = threadIdx.x & 15, bl = threadIdx.x >> 4, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 16 + cl;
  const bool ok = c < N;
  const float* t1 = tab + (ok ? c : 0);
  const float* t2 = t1 + (long)nb * N;
  const int g_lo = PER_GROUP ? (int)blockIdx.y : 0, g_hi = PER_GROUP ? g_lo + 1 : G;
  for (int g = g_lo; g < g_hi; ++g) {
    float a = 0.f, b = 0.f;
    if (unit <= 0) {
      const int b0 = (int)((long)g * group_rows / 128), b1 = (int)((long)(g + 1) * group_rows / 128);
#pragma unroll 4
      for (int k = b0 + bl; k < b1; k += 64) { a += t1[(long)k * N]; b += t2[(long)k * N]; }
    } else {
      const int bpu = unit / 128, total = (int)((long)group_rows / 128);      // blocks of this group: unit u = g + G * (j / bpu)
#pragma unroll 4
      for (int j = bl; j < total; j += 64) {
        const long k = ((long)g + (long)G * (j / bpu)) * bpu + j % bpu;
        a += t1[k * N];
        b += t2[k * N];
      }
    }
    a += __shfl_xor(a, 16); b += __shfl_xor(b, 16);
    a += __shfl_xor(a, 32); b += __shfl_xor(b, 32);
    if ((threadIdx.x & 63) < 16) {
      red[(((g - g_lo) * 2 + 0) * 16 + wave) * 16 + cl] = a;
      red[(((g - g_lo) * 2 + 1) * 16 + wave) * 16 + cl] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 16 || !ok) return;
  float rm = (!PER_GROUP && running_mean) ? running_mean[c] : 0.f, rv = (!PER_GROUP && running_var) ? running_var[c] : 0.f;
  for (int g = g_lo; g < g_hi; ++g) {
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      s += (double)red[(((g - g_lo) * 2 + 0) * 16 + w) * 16 + cl];
      q += (double)red[(((g - g_lo) * 2 + 1) * 16 + w) * 16 + cl];
    }
    const double m = s / group_rows;
    const float var = fmaxf((float)(q / group_rows - m * m), 0.f);
    mean[(long)g * N + c] = (float)m;
    rstd[(long)g * N + c] = rsqrtf(var + eps);
    rm = (1.f - momentum) * rm + momentum * (float)m;
    rv = (1.f - momentum) * rv + momentum * var * ((float)group_rows / (float)max(group_rows - 1, 1));
  }
  if (!PER_GROUP && running_mean) { running_mean[c] = rm; running_var[c] = rv; }
}

// running statistics from per-group mean / rstd, group 0 first (var = 1 / rstd^2 - eps)
__global__ __launch_bounds__(256) void bn_running_update_kernel(const float* mean, const float* rstd, float* running_mean, float* running_var,
                                                                int N, int G, int group_rows, float eps, float momentum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float rm = running_mean[c], rv = running_var[c];
  const float unb = (float)group_rows / (float)max(group_rows - 1, 1);
  for (int g = 0; g < G; ++g) {
    const float r = rstd[(long)g * N + c];
    const float var = fmaxf(1.f / (r * r) - eps, 0.f);
    rm = (1.f - momentum) * rm + momentum * mean[(long)g * N + c];
    rv = (1.f - momentum) * rv + momentum * var * unb;
  }
  running_mean[c] = rm;
  running_var[c] = rv;
}

extern "C" int stswin_bn_table_finalize(const float* table, int M, int N, int groups, int unit_rows, float* mean, float* rstd,
                                        float* running_mean, float* running_var, float eps, float momentum, void* stream) {
  if (M <= 0 || N <= 0 || groups <= 0 || groups > 32 || M % groups) return -1413;      // (32 groups = 64 KB of LDS partials)
  const int gr = M / groups;
  if (unit_rows > 0 ? (unit_rows % 256 || M % ((long)groups * unit_rows)) : (gr % 256)) return -1414;   // whole 256-row tiles per group
  const int nb = 2 * ((M + 255) / 256);
  if (groups > 8) {                                    // the one-launch kernel walks its groups serially: 19.8 us for 24 of them
    hipLaunchKernelGGL(bn_table_finalize_kernel<true>, dim3((unsigned)((N + 15) / 16), (unsigned)groups), dim3(1024), (size_t)2 * 16 * 16 * sizeof(float),
                       (hipStream_t)stream, table, nb, N, groups, gr, unit_rows, mean, rstd, running_mean, running_var, eps, momentum);
    if (running_mean && running_var)
      hipLaunchKernelGGL(bn_running_update_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mean, rstd, running_mean,
                         running_var, N, groups, gr, eps, momentum);
  } else {
    hipLaunchKernelGGL(bn_table_finalize_kernel<false>, dim3((unsigned)((N + 15) / 16)), dim3(1024), (size_t)groups * 2 * 16 * 16 * sizeof(float),
                       (hipStream_t)stream, table, nb, N, groups, gr, unit_rows, mean, rstd, running_mean, running_var, eps, momentum);
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_cs_group_reduce(const float* table, int M, int N, int groups, int unit_rows, float* sum, float* sumsq,
                                      void* stream) {
  if (M <= 0 || N <= 0 || groups <= 0 || M % groups) return -1411;
  const int gr = M / groups;
  if (unit_rows > 0 ? (unit_rows % 256 || M % ((long)groups * unit_rows)) : (gr % 256)) return -1412;   // whole 256-row tiles per group
  const int nb = 2 * ((M + 255) / 256);
  hipLaunchKernelGGL(cs_group_reduce_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)groups), dim3(256), 0, (hipStream_t)stream, table, nb,
                     N, groups, gr, unit_rows, sum, sumsq);
  STSWIN_CHECK_LAUNCH();
  return 0;
}
