// HBM-bound row kernels: window gather / scatter (bit-exact indexing), row-map builders, LayerNorm, column sums.
// Every kernel moves whole 16-byte pieces per lane (8 bf16 / 4 f32), one wave per token row.
#include "common.h"
#include <cstdlib>

// ---------------------------------------------------------------------------------------------------
// Source token of row `r` of the pair-regrouped window layout  (B*nW, T, ws*ws)  <-  (B, T, H*W).
// Restates swin_512.py:210-218: roll(-s,-s) -> window_partition -> view(B,T,nW,N) -> permute(0,2,1,3).
// Returned index is into a token list of `frames_total` frames per clip starting at frame `f0`
// (so a layer that only touches frames 1..2 of a 4-frame clip needs no slice copy).
// ---------------------------------------------------------------------------------------------------
DEVI int win_src_token(int r, int T, int H, int W, int ws, int shift, int f0, int frames_total) {
  const int N = ws * ws, nwx = W / ws, nW = (H / ws) * nwx;
  const int n = r % N; int q = r / N;
  const int t = q % T; q /= T;
  const int wi = q % nW; const int b = q / nW;
  const int ys = (wi / nwx) * ws + n / ws, xs = (wi % nwx) * ws + n % ws;   // position in the rolled image
  int y = ys + shift, x = xs + shift;                                        // rolled[i] = orig[(i+s) mod n]
  if (y >= H) y -= H;
  if (x >= W) x -= W;
  return ((b * frames_total + f0 + t) * H + y) * W + x;
}

__global__ void win_rowmap_kernel(int* map, int rows, int T, int H, int W, int ws, int shift, int f0, int ftot) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) map[r] = win_src_token(r, T, H, W, ws, shift, f0, ftot);
}

// dir = 0: out[r] = in[src(r)]   (gather: a1+a3+a4)      dir = 1: out[src(r)] = in[r]   (scatter: a2+a3^-1)
template <typename T>
__global__ __launch_bounds__(256) void win_move_kernel(const T* in, T* out, int rows, int C, int Tt, int H, int W,
                                                        int ws, int shift, int f0, int ftot, int dir) {
  constexpr int PACK = TT<T>::PACK;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int s = win_src_token(r, Tt, H, W, ws, shift, f0, ftot);
  const long from = dir == 0 ? (long)s : (long)r, to = dir == 0 ? (long)r : (long)s;
  const uint4* src = (const uint4*)(in + from * C);
  uint4* dst = (uint4*)(out + to * C);
  for (int c = threadIdx.x & 63; c < C / PACK; c += 64) dst[c] = src[c];
}

// Patch-merging 2x2 gather map (swin_512.py:267-271): segment order [(0,0),(1,0),(0,1),(1,1)] = (dy,dx).
__global__ void merge_rowmap_kernel(int* map, int frames, int H, int W) {
  const int Ho = H / 2, Wo = W / 2, M = frames * Ho * Wo;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  const int xo = r % Wo, yo = (r / Wo) % Ho, f = r / (Wo * Ho);
  const int dy[4] = {0, 1, 0, 1}, dx[4] = {0, 0, 1, 1};
#pragma unroll
  for (int s = 0; s < 4; ++s) map[s * M + r] = (f * H + 2 * yo + dy[s]) * W + 2 * xo + dx[s];
}

// 3x3 (dilated) convolution tap map: segment s = ky*3+kx -> source pixel or -1 (zero padding = dilation).
__global__ void conv3x3_rowmap_kernel(int* map, int frames, int H, int W, int dil) {
  const int M = frames * H * W;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  const int x = r % W, y = (r / W) % H, f = r / (W * H);
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int yy = y + (s / 3 - 1) * dil, xx = x + (s % 3 - 1) * dil;
    map[s * M + r] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (f * H + yy) * W + xx : -1;
  }
}

// general k x k tap maps (forward gather and its inverse for dgrad)
__global__ void conv_rowmap_kernel(int* map, int frames, int Hin, int Win, int Hout, int Wout, int k, int stride, int pad,
                                   int dil, int inverse) {
  const int Mo = frames * Hout * Wout, Mi = frames * Hin * Win;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (!inverse) {
    if (r >= Mo) return;
    const int x = r % Wout, y = (r / Wout) % Hout, f = r / (Wout * Hout);
    for (int t = 0; t < k * k; ++t) {
      const int yy = y * stride - pad + (t / k) * dil, xx = x * stride - pad + (t % k) * dil;
      map[(long)t * Mo + r] = (yy >= 0 && yy < Hin && xx >= 0 && xx < Win) ? (f * Hin + yy) * Win + xx : -1;
    }
  } else {
    if (r >= Mi) return;
    const int x = r % Win, y = (r / Win) % Hin, f = r / (Win * Hin);
    for (int t = 0; t < k * k; ++t) {
      const int ny = y + pad - (t / k) * dil, nx = x + pad - (t % k) * dil;
      int v = -1;
      if (ny >= 0 && nx >= 0 && ny % stride == 0 && nx % stride == 0) {
        const int yo = ny / stride, xo = nx / stride;
        if (yo < Hout && xo < Wout) v = (f * Hout + yo) * Wout + xo;
      }
      map[(long)t * Mi + r] = v;
    }
  }
}

// stem im2col: a thread owns ONE 16-byte chunk position of the patch row (PACK consecutive columns; column = tap*3 +
// channel, columns >= 147 are the zero padding up to ld) and walks over pixels, so the column -> (dy, dx, channel)
// decode is done once per thread and the row leaves in whole 16-byte stores.  Measured 290-300 us for 403 MB of patches
// in all three variants tried (per-tap 2-byte stores, per-chunk, this one): the bound is the gather itself - a wave load
// touches up to 64 distinct cache lines (taps x channels x pixels) - so the next step would be staging the 7 input rows
// of a pixel strip in LDS.  Runs once per step (the patches are kept for the weight gradient).
template <typename T>
__global__ __launch_bounds__(256) void stem_im2col_kernel(const float* img, T* patches, long ld, int frames, int H, int W,
                                                           int Ho, int Wo) {
  // One workgroup = TP consecutive output pixels of one output row.  The 7 input rows x (2 TP + 5) columns x 3 channels they
  // read are staged in LDS with coalesced loads (zeros outside the image), then every thread assembles 16-byte pieces of
  // patch rows from LDS.  (Reading the taps straight from the NCHW image - eight scattered, bounds-tested 4-byte loads per
  // 16-byte store - ran at 1.4 TB/s of patch writes: 290 us for the 403 MB of a 16-frame 512x512 batch.)
  constexpr int PACK = TT<T>::PACK;
  constexpr int TPMAX = 40, LW = 2 * TPMAX + 8;  // LDS row pitch (floats)
  __shared__ float win[3][7][LW];
  const int cpr = (int)(ld / PACK);              // chunks per row (ld is a multiple of PACK)
  const int ppb = 256 / cpr;                     // pixels per pass
  const int TP = min(TPMAX, 4 * ppb);
  const int tiles_x = (Wo + TP - 1) / TP;
  const int tx = blockIdx.x % tiles_x;
  const int y = (blockIdx.x / tiles_x) % Ho, f = blockIdx.x / (tiles_x * Ho);
  const int x0 = tx * TP, ncols = 2 * TP + 5;
  const float* base = img + (long)f * 3 * H * W;
  for (int i = threadIdx.x; i < 3 * 7 * ncols; i += 256) {
    const int c = i / (7 * ncols), r = (i / ncols) % 7, q = i % ncols;
    const int yy = 2 * y - 3 + r, xx = 2 * x0 - 3 + q;
    win[c][r][q] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? base[((long)c * H + yy) * W + xx] : 0.f;
  }
  __syncthreads();
  const int ch = threadIdx.x % cpr, pl0 = threadIdx.x / cpr;
  if (pl0 >= ppb) return;
  int off[PACK];                                 // LDS offset of tap element e relative to the pixel's window origin, or -1
#pragma unroll
  for (int e = 0; e < PACK; ++e) {
    const int col = ch * PACK + e, t = col / 3, c = col - 3 * t;
    off[e] = t < 49 ? (c * 7 + t / 7) * LW + t % 7 : -1;
  }
  const long row0 = ((long)f * Ho + y) * Wo;
  for (int pl = pl0; pl < TP && x0 + pl < Wo; pl += ppb) {
    Vec16<T> o;
#pragma unroll
    for (int e = 0; e < PACK; ++e) o.set(e, off[e] >= 0 ? (&win[0][0][0])[off[e] + 2 * pl] : 0.f);
    *(decltype(o.v)*)(patches + (row0 + x0 + pl) * ld + ch * PACK) = o.v;
  }
}

// Stem input as a 2 x 2 SPACE-TO-DEPTH image (torchvision conv1 7x7 / 2 / 3 of resnet.py:98-102 as a 4 x 4 convolution of stride 1
// over 12-channel superpixels): record (f, sy, sx) of the padded [F][Ho + 3][Wo + 3] grid (2 records of padding before, 1 after)
// holds the 2 x 2 x 3 input values img[f][c][2 (sy - 2) + dy][2 (sx - 2) + dx] at position (dy * 2 + dx) * 3 + c, then 4 zeros.
// Output pixel (oy, ox) reads the FOUR records (oy + s, ox .. ox + 3) of each tap row s = 0..3: 64 contiguous values - a segment
// the row-map gather of gemm_nt / gemm_tn takes as it is (row pitch 16 < segment length 64: overlapping rows), so neither the
// forward GEMM nor the weight gradient needs the 147-wide patch matrix (403 MB at 16 frames of 512 x 512; this image: 34 MB).
template <typename T>
__global__ __launch_bounds__(256) void stem_s2d_kernel(const float* img, T* out, int frames, int H, int W, int Hs, int Ws) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x, total = (long)frames * Hs * Ws;
  if (n >= total) return;
  const int sx = (int)(n % Ws), sy = (int)((n / Ws) % Hs), f = (int)(n / ((long)Ws * Hs));
  const int iy = 2 * (sy - 2), ix = 2 * (sx - 2);
  float v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = 0.f;
  const float* base = img + (long)f * 3 * H * W;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int y = iy + dy, x = ix + dx;
      if (y >= 0 && y < H && x >= 0 && x < W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[(dy * 2 + dx) * 3 + c] = base[((long)c * H + y) * W + x];
      }
    }
  constexpr int PACK = TT<T>::PACK;
#pragma unroll
  for (int h = 0; h < 16 / PACK; ++h) {
    Vec16<T> o;
#pragma unroll
    for (int e = 0; e < PACK; ++e) o.set(e, v[h * PACK + e]);
    *(decltype(o.v)*)(out + n * 16 + h * PACK) = o.v;
  }
}

// conv weight packing: (Cout, Cin, k, k) fp32 parameter -> the two GEMM operand matrices of the token convolutions in one
// launch: fwd [Cout_p][S][Cin_p] (B operand of y = X W^T, tap-major K) and dgrad [Cin_p][S][Cout_p].  omap / imap give the
// source channel of every padded channel position (-1 = zero padding; concatenated layouts have gaps).  Replaces, per
// convolution and step, a zero fill + slice copies + a cast for each of the two matrices (6 launches of a few us).
// One workgroup = a 64 (out) x 64 (in) channel tile of one tap: the reads run along the input channels, the forward matrix
// is written along them too, and the transposed (dgrad) matrix goes through an LDS tile so that its writes run along the
// output channels.  (One element per thread with a cop-strided 2-byte store for the transposed copy took 1.1 ms per
// training step for the 110 M parameters of TswinPlus - the re-cast happens after every optimizer step.)
template <typename T>
DEVI void conv_pack_tile(T (&tile)[64][66], const float* w, T* fwd, T* dg, const int* omap, const int* imap, int ci, int S, int cop,
                         int cip, int i0, int o0, int s) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  {
    const int ip = i0 + tx;
    const int si = ip < cip ? imap[ip] : -1;
    // three phases, each with its 16 requests in flight together (map entries, weights, stores): as one loop it was 16
    // dependent map -> weight round trips per thread
    int so[16];
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int op = o0 + k * 4 + ty; so[k] = op < cop ? omap[op] : -1; }
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (so[k] >= 0 && si >= 0) ? w[((long)so[k] * ci + si) * S + s] : 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int ol = k * 4 + ty, op = o0 + ol;
      const T o = from_f32<T>(v[k]);
      if (op < cop && ip < cip) fwd[((long)op * S + s) * cip + ip] = o;
      tile[ol][tx] = o;
    }
  }
  if (!dg) return;
  __syncthreads();
  const int op = o0 + tx;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int il = k * 4 + ty, ip = i0 + il;
    if (op < cop && ip < cip) dg[((long)ip * S + s) * cop + op] = tile[tx][il];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* w, T* fwd, T* dg, const int* omap, const int* imap,
                                                         int co, int ci, int S, int cop, int cip) {
  __shared__ T tile[64][66];
  conv_pack_tile<T>(tile, w, fwd, dg, omap, imap, ci, S, cop, cip, blockIdx.x * 64, blockIdx.y * 64, blockIdx.z);
}

// Every convolution weight of a model in ONE launch: the re-cast after an optimizer step was 36 launches of ~15 us for the 36
// convolutions of TswinPlus (and 55 of ~6 us for its Linear weights, below) - kernels far too small to fill the chip, plus a
// launch boundary each.  A workgroup finds its (weight, tile) by scanning the <= 32 tile counts.
#define CPM_MAX 32
struct ConvPackMulti {
  const float* w[CPM_MAX]; void* fwd[CPM_MAX]; void* dg[CPM_MAX]; const int* omap[CPM_MAX]; const int* imap[CPM_MAX];
  int ci[CPM_MAX], S[CPM_MAX], cop[CPM_MAX], cip[CPM_MAX], tiles[CPM_MAX];
  int count;
};
template <typename T>
__global__ __launch_bounds__(256) void conv_pack_multi_kernel(ConvPackMulti a) {
  __shared__ T tile[64][66];
  int b = blockIdx.x, e = 0;
  for (; e < a.count; ++e) {
    if (b < a.tiles[e]) break;
    b -= a.tiles[e];
  }
  if (e >= a.count) return;
  const int ti = (a.cip[e] + 63) / 64, to = (a.cop[e] + 63) / 64;
  const int s = b / (ti * to), r = b - s * ti * to;
  conv_pack_tile<T>(tile, a.w[e], (T*)a.fwd[e], (T*)a.dg[e], a.omap[e], a.imap[e], a.ci[e], a.S[e], a.cop[e], a.cip[e], (r % ti) * 64,
                    (r / ti) * 64, s);
}

// nn.Linear weight [n][k] fp32 -> W (cast) and W^T (cast + transpose) in one launch, 16-byte reads, 8-byte writes: a
// 64 x 64 tile per workgroup, four consecutive elements per thread and pass, the transposed copy through an LDS tile.
template <typename T>
DEVI void linear_pack_tile(float (&tile)[64][65], const float* w, T* fwd, T* tr, int n, int k, int k0, int n0) {
  const int g = threadIdx.x & 15, r = threadIdx.x >> 4;          // 16 groups of 4 columns x 16 rows per pass
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int row = ps * 16 + r, gn = n0 + row, gk = k0 + g * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gn < n && gk < k) {                                        // (k % 4 == 0: whole pieces)
      v = __builtin_nontemporal_load((const f32x4*)(w + (long)gn * k + gk));   // (the fp32 master weights stream through once: repack 0.275 -> 0.263 ms)
      typedef T tx4 __attribute__((ext_vector_type(4)));
      *(tx4*)(fwd + (long)gn * k + gk) = (tx4){from_f32<T>(v[0]), from_f32<T>(v[1]), from_f32<T>(v[2]), from_f32<T>(v[3])};
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[row][g * 4 + e] = v[e];
  }
  if (!tr) return;
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int row = ps * 16 + r, gk = k0 + row, gn = n0 + g * 4;   // output row = input column
    if (gk < k && gn < n) {                                         // (n % 4 == 0)
      typedef T tx4 __attribute__((ext_vector_type(4)));
      *(tx4*)(tr + (long)gk * n + gn) = (tx4){from_f32<T>(tile[g * 4 + 0][row]), from_f32<T>(tile[g * 4 + 1][row]),
                                             from_f32<T>(tile[g * 4 + 2][row]), from_f32<T>(tile[g * 4 + 3][row])};
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void linear_pack_kernel(const float* w, T* fwd, T* tr, int n, int k) {
  __shared__ float tile[64][65];
  linear_pack_tile<T>(tile, w, fwd, tr, n, k, blockIdx.x * 64, blockIdx.y * 64);
}

#define LPM_MAX 64
struct LinearPackMulti {
  const float* w[LPM_MAX]; void* fwd[LPM_MAX]; void* tr[LPM_MAX];
  int n[LPM_MAX], k[LPM_MAX], tiles[LPM_MAX];
  int count;
};
template <typename T>
__global__ __launch_bounds__(256) void linear_pack_multi_kernel(LinearPackMulti a) {
  __shared__ float tile[64][65];
  int b = blockIdx.x, e = 0;
  for (; e < a.count; ++e) {
    if (b < a.tiles[e]) break;
    b -= a.tiles[e];
  }
  if (e >= a.count) return;
  const int tk = (a.k[e] + 63) / 64;
  linear_pack_tile<T>(tile, a.w[e], (T*)a.fwd[e], (T*)a.tr[e], a.n[e], a.k[e], (b % tk) * 64, (b / tk) * 64);
}

// maxpool 3x3 stride 2 pad 1 on tokens
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* in, long ldi, T* out, long ldo, unsigned char* arg,
                                                           int frames, int H, int W, int Ho, int Wo, int C) {
  constexpr int PACK = TT<T>::PACK;
  const int ppr = C / PACK;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)frames * Ho * Wo * ppr) return;
  const int c = (idx % ppr) * PACK;
  const long px = idx / ppr;
  const int x = px % Wo, y = (px / Wo) % Ho, f = px / ((long)Wo * Ho);
  float best[8]; unsigned char ba[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { best[e] = -3.0e38f; ba[e] = 255; }
  for (int t = 0; t < 9; ++t) {
    const int yy = 2 * y - 1 + t / 3, xx = 2 * x - 1 + t % 3;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    Vec16<T> v;
    v.v = *(const decltype(v.v)*)(in + (((long)f * H + yy) * W + xx) * ldi + c);
#pragma unroll
    for (int e = 0; e < PACK; ++e) {
      const float u = v.get(e);
      if (u > best[e] || ba[e] == 255) { best[e] = u; ba[e] = (unsigned char)t; }
    }
  }
  Vec16<T> o;
#pragma unroll
  for (int e = 0; e < PACK; ++e) { o.set(e, best[e]); arg[px * C + c + e] = ba[e]; }
  *(decltype(o.v)*)(out + px * ldo + c) = o.v;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* dout, long ldo, T* din, long ldi, const unsigned char* arg,
                                                           int frames, int H, int W, int Ho, int Wo, int C) {
  constexpr int PACK = TT<T>::PACK;
  const int ppr = C / PACK;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)frames * H * W * ppr) return;
  const int c = (idx % ppr) * PACK;
  const long px = idx / ppr;
  const int x = px % W, y = (px / W) % H, f = px / ((long)W * H);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // output pixel (yo, xo) reads (y, x) through tap (ty, tx) iff 2 yo - 1 + ty == y: an odd coordinate has the candidates ty = 0 and
  // ty = 2, an even one only ty = 1 - at most four output pixels, visited in tap order; their winning-tap bytes come in one load
  const int ny = (y & 1) ? 2 : 1, nx = (x & 1) ? 2 : 1;
  for (int iy = 0; iy < ny; ++iy) {
    const int ty = (y & 1) ? 2 * iy : 1, yo = (y + 1 - ty) >> 1;
    if (yo >= Ho) continue;
    for (int ix = 0; ix < nx; ++ix) {
      const int tx = (x & 1) ? 2 * ix : 1, xo = (x + 1 - tx) >> 1;
      if (xo >= Wo) continue;
      const unsigned t = (unsigned)(ty * 3 + tx);
      const long po = ((long)f * Ho + yo) * Wo + xo;
      Vec16<T> d;
      d.v = *(const decltype(d.v)*)(dout + po * ldo + c);
      unsigned a[2] = {0, 0};
      if (PACK == 8) { const uint2 w = *(const uint2*)(arg + po * C + c); a[0] = w.x; a[1] = w.y; }
      else a[0] = *(const unsigned*)(arg + po * C + c);
#pragma unroll
      for (int e = 0; e < PACK; ++e)
        if (((a[e >> 2] >> (8 * (e & 3))) & 0xFFu) == t) acc[e] += d.get(e);
    }
  }
  Vec16<T> o;
#pragma unroll
  for (int e = 0; e < PACK; ++e) o.set(e, acc[e]);
  *(decltype(o.v)*)(din + px * ldi + c) = o.v;
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm over rows that may be the concatenation of S gathered segments (patch merging: S = 4).
// One wave per row; the row lives in registers (C <= 4096); statistics two-pass in fp32 like torch.
// ---------------------------------------------------------------------------------------------------
template <typename T, int NP>   // NP = pieces of 16 B per lane
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* x, long ldx, const int* rows, int S, int Cseg, T* y,
                                                      long ldy, const float* gamma, const float* beta, float* mean,
                                                      float* rstd, int M, float eps) {
  constexpr int PACK = TT<T>::PACK;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (r >= M) return;
  const int C = S * Cseg;
  float v[NP][PACK];
  float sum = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = (p * 64 + l) * PACK;
    if (c < C) {
      const int s = c / Cseg, cc = c - s * Cseg;
      const long row = rows ? (long)rows[(long)s * M + r] : (long)r;
      Vec16<T> in;
      in.v = *(const decltype(in.v)*)(x + row * ldx + cc);
#pragma unroll
      for (int e = 0; e < PACK; ++e) { v[p][e] = in.get(e); sum += v[p][e]; }
    } else {
#pragma unroll
      for (int e = 0; e < PACK; ++e) v[p][e] = 0.f;
    }
  }
  const float mu = wave_sum(sum) / C;
  float sq = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = (p * 64 + l) * PACK;
    if (c < C) {
#pragma unroll
      for (int e = 0; e < PACK; ++e) { const float d = v[p][e] - mu; sq += d * d; }
    }
  }
  const float rs = rsqrtf(wave_sum(sq) / C + eps);
  if (l == 0 && mean) { mean[r] = mu; rstd[r] = rs; }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = (p * 64 + l) * PACK;
    if (c < C) {
      Vec16<T> o;
#pragma unroll
      for (int e = 0; e < PACK; ++e) o.set(e, (v[p][e] - mu) * rs * gamma[c + e] + beta[c + e]);
      *(decltype(o.v)*)(y + (long)r * ldy + c) = o.v;
    }
  }
}

// ---- deterministic cross-workgroup sums ---------------------------------------------------------------------------------
// Every kernel of this library that sums over workgroups (bias / LayerNorm / BatchNorm parameter gradients, BatchNorm
// statistics, the relative-position-bias gradient) writes ONE partial vector per workgroup with plain stores ("slab" p of a
// caller-owned scratch buffer) and this kernel adds the slabs in a fixed order behind the launch boundary: no fp32 atomics,
// so the results do not depend on the order in which workgroups happen to finish - two runs of a training step give the same
// bits.  (Same-address fp32 atomics also serialise at ~40 ns each.)
//   out_s[b * obs_s + j] (+)= sum_{p < nslabs} ws[b * ws_batch_stride + p * slab_stride + off_s + j],  j < len_s, off_s = len_0 + .. + len_{s-1}
// for up to three output vectors s (lengths multiples of 4).  Block: 16 float4 columns x 16 slab lanes; lane q adds the slabs
// q, q + 16, ... and the 16 lane sums are added in lane order.
struct FoldArgs {
  const float* ws; long slab_stride, ws_batch_stride; int nslabs;
  int len[3]; float* out[3]; long obs[3]; int accumulate, cl;
};
// cl = float4 columns per workgroup (16: few slabs, 64 floats per workgroup; 4: many slabs - 64 slab lanes per column, four times
// the workgroups); the association of the sum is fixed by (nslabs, cl) alone.
DEVI void slab_fold_body(const FoldArgs& f, int block_x, int batch) {
  __shared__ f32x4 fold[256];
  const int CL = f.cl, QL = 256 / CL;
  const int cl = threadIdx.x % CL, q = threadIdx.x / CL;
  const int j = (block_x * CL + cl) * 4;
  const bool in = j < f.len[0] + f.len[1] + f.len[2];
  const float* src = f.ws + (long)batch * f.ws_batch_stride + j;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (in) {
    int p = q;
    for (; p + 3 * QL < f.nslabs; p += 4 * QL) {             // four independent loads in flight per lane
      const f32x4 v0 = *(const f32x4*)(src + (long)p * f.slab_stride), v1 = *(const f32x4*)(src + (long)(p + QL) * f.slab_stride);
      const f32x4 v2 = *(const f32x4*)(src + (long)(p + 2 * QL) * f.slab_stride), v3 = *(const f32x4*)(src + (long)(p + 3 * QL) * f.slab_stride);
      a += v0; a += v1; a += v2; a += v3;
    }
    for (; p < f.nslabs; p += QL) a += *(const f32x4*)(src + (long)p * f.slab_stride);
  }
  fold[q * CL + cl] = a;
  __syncthreads();
  if (q == 0 && in) {
    for (int k = 1; k < QL; ++k) a += fold[k * CL + cl];
    const int sgm = j < f.len[0] ? 0 : (j < f.len[0] + f.len[1] ? 1 : 2);
    const int jj = j - (sgm > 0 ? f.len[0] : 0) - (sgm > 1 ? f.len[1] : 0);
    float* out = f.out[sgm];
    if (out) {
      f32x4* dst = (f32x4*)(out + (long)batch * f.obs[sgm] + jj);
      *dst = f.accumulate ? *dst + a : a;
    }
  }
}
__global__ __launch_bounds__(256) void slab_fold_kernel(FoldArgs f) { slab_fold_body(f, blockIdx.x, blockIdx.y); }

// Several folds in ONE launch (stswin_fold_defer / stswin_fold_flush): a backward pass of a Swin block queues the folds of its two
// LayerNorm backward passes, its bias-gradient tables and the attention kernel's slabs - none of their results is read before the
// pass ends - and launches them together (4 launches of ~5 us less per block and step).
#define FOLD_QUEUE_MAX 12
struct FoldBatch { FoldArgs f[FOLD_QUEUE_MAX]; int first_block[FOLD_QUEUE_MAX + 1]; int blocks_x[FOLD_QUEUE_MAX]; int count; };
__global__ __launch_bounds__(256) void slab_fold_multi_kernel(FoldBatch b) {
  int i = 0;
  while (i + 1 < b.count && (int)blockIdx.x >= b.first_block[i + 1]) ++i;
  const int local = blockIdx.x - b.first_block[i];
  slab_fold_body(b.f[i], local % b.blocks_x[i], local / b.blocks_x[i]);
}
static thread_local int g_fold_defer = 0;
static thread_local FoldBatch g_fold_batch;

static int fold_flush(hipStream_t st) {
  FoldBatch& b = g_fold_batch;
  if (b.count > 0) {
    hipLaunchKernelGGL(slab_fold_multi_kernel, dim3((unsigned)b.first_block[b.count]), dim3(256), 0, st, b);
    b.count = 0;
  }
  return 0;
}
extern "C" int stswin_fold_defer(int on, void* stream) {          // on = 0 flushes what is queued
  if (!on) { fold_flush((hipStream_t)stream); g_fold_defer = 0; STSWIN_CHECK_LAUNCH(); return 0; }
  g_fold_defer = 1;
  g_fold_batch.count = 0;
  return 0;
}
extern "C" int stswin_fold_flush(void* stream) {
  fold_flush((hipStream_t)stream);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

int stswin_fold3_launch(const float* ws, long slab_stride, long ws_batch_stride, int nslabs, const int* len, float* const* out,
                        const long* obs, int batch, int accumulate, hipStream_t st) {
  FoldArgs f;
  f.ws = ws; f.slab_stride = slab_stride; f.ws_batch_stride = ws_batch_stride; f.nslabs = nslabs; f.accumulate = accumulate;
  int tot = 0;
  for (int i = 0; i < 3; ++i) {
    f.len[i] = len[i]; f.out[i] = out[i]; f.obs[i] = obs[i];
    if (len[i] < 0 || len[i] % 4 || obs[i] % 4) return -1110;
    tot += len[i];
  }
  if (nslabs <= 0 || tot <= 0 || batch <= 0) return 0;
  if (slab_stride % 4 || ws_batch_stride % 4) return -1110;
  f.cl = nslabs >= 96 ? 4 : 16;
  const int bx = (tot + 4 * f.cl - 1) / (4 * f.cl);
  if (g_fold_defer) {
    FoldBatch& b = g_fold_batch;
    if (b.count == FOLD_QUEUE_MAX) fold_flush(st);
    if (b.count == 0) b.first_block[0] = 0;
    b.f[b.count] = f; b.blocks_x[b.count] = bx;
    b.first_block[b.count + 1] = b.first_block[b.count] + bx * batch;
    ++b.count;
    return 0;
  }
  hipLaunchKernelGGL(slab_fold_kernel, dim3((unsigned)bx, (unsigned)batch), dim3(256), 0, st, f);
  return 0;
}

int stswin_fold_launch(const float* ws, long slab_stride, long ws_batch_stride, int nslabs, int seg_len, int nseg, float* o0, float* o1,
                       float* o2, long out_batch_stride, int batch, int accumulate, hipStream_t st) {
  if (nseg <= 0 || nseg > 3 || seg_len <= 0) return nseg > 3 ? -1110 : 0;
  const int len[3] = {seg_len, nseg > 1 ? seg_len : 0, nseg > 2 ? seg_len : 0};
  float* const out[3] = {o0, o1, o2};
  const long obs[3] = {out_batch_stride, out_batch_stride, out_batch_stride};
  return stswin_fold3_launch(ws, slab_stride, ws_batch_stride, nslabs, len, out, obs, batch, accumulate, st);
}

// dx = rstd * (g*dy - mean(g*dy) - xhat * mean(g*dy*xhat));  dgamma += sum dy*xhat ; dbeta += sum dy.
// Each wave walks `rows_per_wave` consecutive rows keeping its dgamma/dbeta columns in registers, the block
// folds its NW waves through LDS and stores one partial row per workgroup (summed by slab_fold_kernel).
// Round 5 (profiles/r05_layernorm_kernels.txt): ALL pieces of a row - x, dy, the old dx when accumulating, mean, rstd - are
// requested before the first one is used (inside the per-piece `if (c < C)` bodies hipcc kept each piece's loads behind the
// previous piece's arithmetic: one round trip per piece), gamma is read from LDS (as global loads its pieces were re-requested for
// every row), "accumulate" and "column sums of dx" are template switches (C = 2048 had spilled), and workgroups are 8 waves where
// four would leave the grid at <= 512 workgroups.  C = 1024: 35.5 -> 30.9 us, C = 2048 gathered: 113 -> 70 us; C = 512 unchanged
// (one piece per row; ~200 VALU instructions per row and wave make that launch as much VALU- as HBM-bound).  Measured and NOT
// kept: the next row prefetched behind the current one, 2 or 4 rows of a wave in flight together (138-186 registers, C = 512
// 50 -> 68 us), g / xhat forcibly re-derived in the second pass (more VALU work), fused multiply-adds (no change).
template <typename T, int NP, int NW, bool ACC, bool DXS>
__global__ __launch_bounds__(NW * 64) void ln_bwd_kernel(const T* dy, long lddy, const T* x, long ldx, const int* rows,
                                                          int S, int Cseg, const float* gamma, const float* mean,
                                                          const float* rstd, T* dx, long lddx, float* dgamma,
                                                          float* dbeta, int M, int rows_per_wave, float* ws,
                                                          const T* add, long ldadd) {      // ACC: dx = add + LN'(dy) (add may be dx itself)
  constexpr int PACK = TT<T>::PACK;
  typedef decltype(Vec16<T>().v) vec_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int C = S * Cseg;
  float dg[NP][PACK], db[NP][PACK], ds[DXS ? NP : 1][PACK];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < PACK; ++e) { dg[p][e] = 0.f; db[p][e] = 0.f; if (DXS) ds[p][e] = 0.f; }
  float* sgam = (float*)smem + NW * C;
  for (int c = threadIdx.x; c < C; c += NW * 64) sgam[c] = gamma[c];
  __syncthreads();
  // workgroups walk row groups blockIdx.x, blockIdx.x + gridDim.x, ... (the launcher caps the grid at 1024: the parameter-gradient
  // partial sums stay in registers across a workgroup's groups, so there is one slab per workgroup to fold afterwards)
  typedef f32x4 raw_t;                 // 16 bytes of a row as a register quad
  constexpr bool EARLY = ACC && NP <= 4;      // (NP = 8: the row's own pieces fill the register file)
  struct Row { raw_t xi[NP], di[NP], old[EARLY ? NP : 1]; float mu, rs; };
  for (int rg = blockIdx.x; rg * NW * rows_per_wave < M; rg += gridDim.x) {
  const int r_begin = (rg * NW + w) * rows_per_wave;
  for (int r = r_begin; r < min(M, r_begin + rows_per_wave); ++r) {
    // every piece of the row is requested up front - the old dx, too, when accumulating (requested where it is used it cost a
    // second round trip per row)
    Row cur;
    cur.mu = mean[r]; cur.rs = rstd[r];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int c = (p * 64 + l) * PACK;
      if (c < C) {
        const int s = c / Cseg, cc = c - s * Cseg;
        const long row = rows ? (long)rows[(long)s * M + r] : (long)r;
        cur.xi[p] = *(const raw_t*)(x + row * ldx + cc);
        cur.di[p] = *(const raw_t*)(dy + (long)r * lddy + c);
        if constexpr (EARLY) cur.old[p] = *(const raw_t*)(add + row * ldadd + cc);
      }
    }
    const float mu = cur.mu, rs = cur.rs;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int c = (p * 64 + l) * PACK;
      if (c < C) {
        Vec16<T> xi, di;
        xi.v = __builtin_bit_cast(vec_t, cur.xi[p]); di.v = __builtin_bit_cast(vec_t, cur.di[p]);
        float gm[PACK];
#pragma unroll
        for (int e = 0; e < PACK; e += 4) *(f32x4*)(gm + e) = *(const f32x4*)(sgam + c + e);
#pragma unroll
        for (int e = 0; e < PACK; ++e) {
          const float d = di.get(e);
          const float xh = (xi.get(e) - mu) * rs;
          const float g = d * gm[e];
          s1 += g;
          s2 += g * xh;
          dg[p][e] += d * xh;
          db[p][e] += d;
        }
      }
    }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
    // (g and xhat are written out again from the row's pieces; hipcc decides per instantiation whether to keep the first pass's
    // floats or to re-derive them)
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int c = (p * 64 + l) * PACK;
      if (c < C) {
        const int s = c / Cseg, cc = c - s * Cseg;
        const long row = rows ? (long)rows[(long)s * M + r] : (long)r;
        T* dst = dx + row * lddx + cc;
        Vec16<T> xi, di, o;
        xi.v = __builtin_bit_cast(vec_t, cur.xi[p]); di.v = __builtin_bit_cast(vec_t, cur.di[p]);
        if constexpr (EARLY) o.v = __builtin_bit_cast(vec_t, cur.old[p]);
        else if constexpr (ACC) o.v = *(const vec_t*)(add + row * ldadd + cc);
        float gm[PACK];
#pragma unroll
        for (int e = 0; e < PACK; e += 4) *(f32x4*)(gm + e) = *(const f32x4*)(sgam + c + e);
#pragma unroll
        for (int e = 0; e < PACK; ++e) {
          const float xh = (xi.get(e) - mu) * rs;
          const float g = di.get(e) * gm[e];
          const float val = rs * (g - s1 - xh * s2);
          const float fin = ACC ? o.get(e) + val : val;
          o.set(e, fin);
          if constexpr (DXS) ds[p][e] += fin;
        }
        *(vec_t*)dst = o.v;
      }
    }
  }
  }
  // fold the NW waves through ONE [NW][C] LDS table, a vector at a time; slab `blockIdx.x` of the caller's scratch:
  // [3][C] = dgamma | dbeta | dxsum partial sums of this workgroup's rows (plain stores; slab_fold_kernel adds the slabs in order
  // afterwards: deterministic, and no same-address atomics)
  float* sg = (float*)smem;
  float* rep = ws + (long)blockIdx.x * 3 * C;
  auto fold = [&](const float (&acc)[NP][PACK], float* out) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int c = (p * 64 + l) * PACK;
      if (c < C) {
#pragma unroll
        for (int e = 0; e < PACK; ++e) sg[w * C + c + e] = acc[p][e];
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NW * 64) {
      float t = sg[c];
#pragma unroll
      for (int k = 1; k < NW; ++k) t += sg[k * C + c];
      out[c] = t;
    }
    __syncthreads();
  };
  fold(dg, rep);
  fold(db, rep + C);
  if constexpr (DXS) fold(ds, rep + 2 * C);     // column sums of dx before its rounding to T (= the bias gradient of the Linear that produced x)
}

// part[blockIdx.y][n] = sum of rows [blockIdx.y * rows_per_block, ...) of Y[:, n]   (bias gradients; slab_fold_kernel adds the
// row-block partials into out).  Block = 256 threads: 32 column-pieces x 8 row lanes.
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* y, long ldy, float* part, int M, int N, int rows_per_block) {
  constexpr int PACK = TT<T>::PACK;
  __shared__ float red[8][32 * 8];
  const int cp = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cp) * PACK;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int r0 = blockIdx.y * rows_per_block;
  if (c < N) {
    for (int r = r0 + rl; r < min(M, r0 + rows_per_block); r += 8) {
      Vec16<T> in;
      in.v = *(const decltype(in.v)*)(y + (long)r * ldy + c);
#pragma unroll
      for (int e = 0; e < PACK; ++e) acc[e] += in.get(e);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cp * 8 + e] = acc[e];
  __syncthreads();
  if (rl == 0 && c < N) {
#pragma unroll
    for (int e = 0; e < PACK; ++e) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t += red[k][cp * 8 + e];
      part[(long)blockIdx.y * N + c + e] = t;
    }
  }
}

// out[i] = map[i] >= 0 ? v[map[i]] : fill   (channel-padding / un-padding of per-channel vectors: one launch instead of a
// fill plus one copy per layout segment)
__global__ __launch_bounds__(256) void vec_gather_kernel(const float* v, const int* map, float* out, int n, float fill) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) { const int j = map[i]; out[i] = j >= 0 ? v[j] : fill; }
}

// the same for up to four vectors that share the map (a BatchNorm's weight | bias | running mean | running variance, or its two
// parameter gradients): one launch instead of four, blockIdx.y = vector
struct VecGatherMulti { const float* v[4]; float* out[4]; float fill[4]; const int* map; int n; };
__global__ __launch_bounds__(256) void vec_gather_multi_kernel(VecGatherMulti p) {
  const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (i < p.n) { const int j = p.map[i]; p.out[k][i] = j >= 0 ? p.v[k][j] : p.fill[k]; }
}

// ---- relative position bias (swin_512.py:122-131): table[index] -> the attention kernels' [key][query] layout, with the
// SW-MSA mask folded in per window, and the transposed scatter of its gradient.  One launch each instead of the
// index / permute / contiguous / add chain (6 tiny kernels per block forward, index_add_ + permute per backward).
__global__ __launch_bounds__(256) void bias_expand_kernel(const float* table, const long* index, const float* mask, float* out,
                                                          int N, int heads, int nW) {
  const long n = (long)nW * heads * N * N;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long)gridDim.x * 256) {
    const int i = (int)(t % N), j = (int)((t / N) % N);          // out[w][h][key j][query i]
    const int h = (int)((t / ((long)N * N)) % heads), w = (int)(t / ((long)N * N * heads));
    float v = table[index[(long)i * N + j] * heads + h];
    if (mask) v += mask[((long)w * N + i) * N + j];
    out[t] = v;
  }
}
// the same for up to 16 tables at once (every Swin block's table after an optimizer step: ops.repack), blockIdx.y = table
#define BEM_MAX 16
struct BiasExpandMulti { const float* table[BEM_MAX]; const long* index[BEM_MAX]; const float* mask[BEM_MAX]; float* out[BEM_MAX];
                         int N[BEM_MAX], heads[BEM_MAX], nW[BEM_MAX]; };
__global__ __launch_bounds__(256) void bias_expand_multi_kernel(BiasExpandMulti p) {
  const int e = blockIdx.y, N = p.N[e], heads = p.heads[e];
  const float* table = p.table[e]; const long* index = p.index[e]; const float* mask = p.mask[e]; float* out = p.out[e];
  const long n = (long)p.nW[e] * heads * N * N;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long)gridDim.x * 256) {
    const int i = (int)(t % N), j = (int)((t / N) % N);
    const int h = (int)((t / ((long)N * N)) % heads), w = (int)(t / ((long)N * N * heads));
    float v = table[index[(long)i * N + j] * heads + h];
    if (mask) v += mask[((long)w * N + i) * N + j];
    out[t] = v;
  }
}
// Gradient of the gather, in gather form (deterministic: no atomics).  `order` lists the (query i, key j) pairs (as i * N + j) sorted
// by their table row, `offs[e] .. offs[e + 1]` is row e's range (both built once per relative_position_index buffer by the
// caller): thread (e, h) adds its <= N pairs in list order.  nslabs > 1: dbiasT is [nslabs][heads][N][N] and the slabs are added on
// the way.
__global__ __launch_bounds__(256) void bias_scatter_kernel(const float* dbiasT, const int* order, const int* offs, float* dtable, int N,
                                                            int heads, int table_rows, int nslabs) {
  // one WAVE per (table row e, head h): lane q adds the pairs q, q + 64, ... of the row (<= N of them for a real index), then a fixed
  // butterfly over the lanes - the per-thread loop of dependent (order -> value) loads was latency-bound (17 us for 900 threads)
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (t >= table_rows * heads) return;
  const int e = t / heads, h = t - e * heads;
  const long NN = (long)N * N;
  float acc = 0.f;
  for (int q = offs[e] + l; q < offs[e + 1]; q += 64) {
    const int pr = order[q], i = pr / N, j = pr - i * N;
    const float* src = dbiasT + ((long)h * N + j) * N + i;        // dbiasT[h][key j][query i]
    for (int sl = 0; sl < nslabs; ++sl) acc += src[(long)sl * heads * NN];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (l == 0) dtable[(long)e * heads + h] += acc;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int stswin_win_rowmap(int* map, int B, int T, int H, int W, int ws, int shift, int f0, int frames_total,
                                 void* stream) {
  if (H % ws || W % ws || shift < 0 || shift >= ws) return -1101;
  const int rows = B * T * H * W;
  hipLaunchKernelGGL(win_rowmap_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, map, rows, T, H, W,
                     ws, shift, f0, frames_total);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_win_move(int dtype, const void* in, void* out, int B, int T, int H, int W, int C, int ws, int shift,
                               int f0, int frames_total, int dir, void* stream) {
  if (H % ws || W % ws || shift < 0 || shift >= ws) return -1101;
  if (C % (dtype == 0 ? 8 : 4)) return -1102;
  const int rows = B * T * H * W;
  if (dtype == 0)
    hipLaunchKernelGGL(win_move_kernel<bf16>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)in,
                       (bf16*)out, rows, C, T, H, W, ws, shift, f0, frames_total, dir);
  else
    hipLaunchKernelGGL(win_move_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float*)in,
                       (float*)out, rows, C, T, H, W, ws, shift, f0, frames_total, dir);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_merge_rowmap(int* map, int frames, int H, int W, void* stream) {
  if ((H | W) & 1) return -1103;
  const int M = frames * (H / 2) * (W / 2);
  hipLaunchKernelGGL(merge_rowmap_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, map, frames, H, W);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_conv3x3_rowmap(int* map, int frames, int H, int W, int dilation, void* stream) {
  const int M = frames * H * W;
  hipLaunchKernelGGL(conv3x3_rowmap_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, map, frames, H, W,
                     dilation);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_conv_rowmap(int* map, int frames, int Hin, int Win, int Hout, int Wout, int k, int stride, int pad,
                                  int dilation, int inverse, void* stream) {
  if (k <= 0 || stride <= 0) return -1108;
  const int n = inverse ? frames * Hin * Win : frames * Hout * Wout;
  hipLaunchKernelGGL(conv_rowmap_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, map, frames, Hin, Win,
                     Hout, Wout, k, stride, pad, dilation, inverse);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_stem_im2col(int dtype, const float* img, void* patches, long ld, int frames, int H, int W, int Ho,
                                  int Wo, void* stream) {
  if (ld < 147 || ld > 192) return -1109;
  const int pk_ = dtype == 0 ? 8 : 4;
  if (ld % pk_) return -1109;
  const int ppb = 256 / (int)(ld / pk_), TP = 4 * ppb < 40 ? 4 * ppb : 40;        // must match the kernel
  const long want = (long)frames * Ho * ((Wo + TP - 1) / TP);
  if (want > 0x7fffffffL) return -1109;
  dim3 grid((unsigned)want);
  if (dtype == 0) hipLaunchKernelGGL(stem_im2col_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, img, (bf16*)patches, ld, frames, H, W, Ho, Wo);
  else hipLaunchKernelGGL(stem_im2col_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, img, (float*)patches, ld, frames, H, W, Ho, Wo);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_stem_s2d(int dtype, const float* img, void* out, int frames, int H, int W, void* stream) {
  if (frames <= 0 || H <= 0 || W <= 0) return -1112;
  const int Hs = (H - 1) / 2 + 1 + 3, Ws = (W - 1) / 2 + 1 + 3;
  const long total = (long)frames * Hs * Ws;
  if (total > 0x7fffffffL * 64) return -1112;
  dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(stem_s2d_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, img, (bf16*)out, frames, H, W, Hs, Ws);
  else hipLaunchKernelGGL(stem_s2d_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, img, (float*)out, frames, H, W, Hs, Ws);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_conv_pack(int dtype, const float* w, void* fwd, void* dgrad, const int* omap, const int* imap, int co,
                                int ci, int S, int cop, int cip, void* stream) {
  if (co <= 0 || ci <= 0 || S <= 0 || cop <= 0 || cip <= 0) return -1111;
  if (S > 65535) return -1111;
  dim3 grid((unsigned)((cip + 63) / 64), (unsigned)((cop + 63) / 64), (unsigned)S);
  if (dtype == 0) hipLaunchKernelGGL(conv_pack_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, w, (bf16*)fwd, (bf16*)dgrad, omap, imap, co, ci, S, cop, cip);
  else hipLaunchKernelGGL(conv_pack_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, w, (float*)fwd, (float*)dgrad, omap, imap, co, ci, S, cop, cip);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_maxpool3x3s2(int dtype, const void* in, long ldi, void* out, long ldo, unsigned char* arg, int frames,
                                   int H, int W, int Ho, int Wo, int C, int backward, void* stream) {
  const int pk = dtype == 0 ? 8 : 4;
  if (C % pk || ldi % pk || ldo % pk) return -1110;
  hipStream_t st = (hipStream_t)stream;
  if (!backward) {
    const long n = (long)frames * Ho * Wo * (C / pk);
    dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == 0) hipLaunchKernelGGL(maxpool_fwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)in, ldi, (bf16*)out, ldo, arg, frames, H, W, Ho, Wo, C);
    else hipLaunchKernelGGL(maxpool_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)in, ldi, (float*)out, ldo, arg, frames, H, W, Ho, Wo, C);
  } else {   /* in = d(out) [F*Ho*Wo][C] (pitch ldi), out = d(in) [F*H*W][C] (pitch ldo) */
    const long n = (long)frames * H * W * (C / pk);
    dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == 0) hipLaunchKernelGGL(maxpool_bwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)in, ldi, (bf16*)out, ldo, arg, frames, H, W, Ho, Wo, C);
    else hipLaunchKernelGGL(maxpool_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)in, ldi, (float*)out, ldo, arg, frames, H, W, Ho, Wo, C);
  }
  STSWIN_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int ln_fwd_launch(const void* x, long ldx, const int* rows, int S, int Cseg, void* y, long ldy, const float* g,
                         const float* b, float* mean, float* rstd, int M, float eps, hipStream_t st) {
  constexpr int PACK = TT<T>::PACK;
  const int C = S * Cseg, np = (C / PACK + 63) / 64;
  dim3 grid((M + 3) / 4), blk(256);
#define LN_F(NP) hipLaunchKernelGGL((ln_fwd_kernel<T, NP>), grid, blk, 0, st, (const T*)x, ldx, rows, S, Cseg, (T*)y, ldy, g, b, mean, rstd, M, eps)
  switch (np) {
    case 1: LN_F(1); break;
    case 2: LN_F(2); break;
    case 3: case 4: LN_F(4); break;
    case 5: case 6: case 7: case 8: LN_F(8); break;
    default:
      if (np <= 16) { LN_F(16); break; }
      return -1104;
  }
#undef LN_F
  return 0;
}

extern "C" int stswin_layernorm_fwd(int dtype, const void* x, long ldx, const int* rows, int S, int Cseg, void* y,
                                    long ldy, const float* gamma, const float* beta, float* mean, float* rstd, int M,
                                    float eps, void* stream) {
  const int pack = dtype == 0 ? 8 : 4;
  if (Cseg % pack || ldx % pack || ldy % pack) return -1105;
  int rc = dtype == 0 ? ln_fwd_launch<bf16>(x, ldx, rows, S, Cseg, y, ldy, gamma, beta, mean, rstd, M, eps, (hipStream_t)stream)
                      : ln_fwd_launch<float>(x, ldx, rows, S, Cseg, y, ldy, gamma, beta, mean, rstd, M, eps, (hipStream_t)stream);
  if (rc) return rc;
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Geometry: 8 rows per wave (M >= 16384); workgroups of 8 waves when four would leave the grid at <= 512 workgroups (C >= 1024 in
// the step: M = 16384), so that 4 waves per SIMD are resident without more slabs to fold; grid capped at 1024.
static int ln_bwd_rows_per_wave(int M) { return M >= 16384 ? 8 : (M >= 4096 ? 4 : 2); }
static int ln_bwd_waves(int M, int C, int pack) {
  const int np = (C / pack + 63) / 64;
  static const char* e = getenv("STSWIN_LN_BWD_WAVES");     // A/B switch (tools/bench_ln.py): 4 or 8
  if (e && (atoi(e) == 4 || atoi(e) == 8)) return np <= 2 ? atoi(e) : 4;
  const int rpw = ln_bwd_rows_per_wave(M);
  return (M + 4 * rpw - 1) / (4 * rpw) <= 512 && M >= 8 * rpw * 128 && np <= 2 ? 8 : 4;
}
static int ln_bwd_grid(int M, int C, int pack) {
  const int rpw = ln_bwd_rows_per_wave(M), nw = ln_bwd_waves(M, C, pack), groups = (M + nw * rpw - 1) / (nw * rpw);
  return groups < 1024 ? groups : 1024;
}
extern "C" long stswin_layernorm_bwd_scratch(int M, int C) {      // (sized for the 4-wave geometry: the larger of the two)
  const int rpw = ln_bwd_rows_per_wave(M), groups = (M + 4 * rpw - 1) / (4 * rpw);
  return (long)(groups < 1024 ? groups : 1024) * 3 * C;
}

template <typename T>
static int ln_bwd_launch(const void* dy, long lddy, const void* x, long ldx, const int* rows, int S, int Cseg,
                         const float* g, const float* mean, const float* rstd, void* dx, long lddx, float* dg, float* db,
                         int M, int acc, float* dxsum, float* ws, hipStream_t st, const void* add = nullptr, long ldadd = 0) {
  if (acc && !add) { add = dx; ldadd = lddx; }
  constexpr int PACK = TT<T>::PACK;
  const int C = S * Cseg, np = (C / PACK + 63) / 64;
  const int rpw = ln_bwd_rows_per_wave(M), nw = ln_bwd_waves(M, C, PACK);
  dim3 grid((unsigned)ln_bwd_grid(M, C, PACK)), blk(nw * 64);
  const size_t lds = (size_t)(nw + 1) * C * sizeof(float);
  if (!ws) return -1111;
#define LN_B4(NP, NW, A, D) hipLaunchKernelGGL((ln_bwd_kernel<T, NP, NW, A, D>), grid, blk, lds, st, (const T*)dy, lddy, (const T*)x, ldx, rows, S, Cseg, g, mean, rstd, (T*)dx, lddx, dg, db, M, rpw, ws, (const T*)add, ldadd)
#define LN_B2(NP, NW) do { if (acc) { if (dxsum) LN_B4(NP, NW, true, true); else LN_B4(NP, NW, true, false); } \
                           else { if (dxsum) LN_B4(NP, NW, false, true); else LN_B4(NP, NW, false, false); } } while (0)
#define LN_B(NP) do { if (nw == 8) LN_B2(NP, 8); else LN_B2(NP, 4); } while (0)
#define LN_BW4(NP) LN_B2(NP, 4)
  switch (np) {
    case 1: LN_B(1); break;
    case 2: LN_B(2); break;
    case 3: case 4: LN_BW4(4); break;
    case 5: case 6: case 7: case 8: LN_BW4(8); break;
    default: return -1104;
  }
#undef LN_B
#undef LN_BW4
#undef LN_B2
#undef LN_B4
  return stswin_fold_launch(ws, 3L * C, 0, (int)grid.x, C, dxsum ? 3 : 2, dg, db, dxsum, 0, 1, 1, st);
}

extern "C" int stswin_layernorm_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, const int* rows, int S,
                                    int Cseg, const float* gamma, const float* mean, const float* rstd, void* dx,
                                    long lddx, float* dgamma, float* dbeta, int M, int accumulate_dx, float* dxsum,
                                    float* workspace, void* stream) {
  const int pack = dtype == 0 ? 8 : 4;
  if (Cseg % pack || ldx % pack || lddy % pack || lddx % pack) return -1105;
  if ((long)S * Cseg * 5 * 4 > 65536) return -1106;
  int rc = dtype == 0 ? ln_bwd_launch<bf16>(dy, lddy, x, ldx, rows, S, Cseg, gamma, mean, rstd, dx, lddx, dgamma, dbeta, M, accumulate_dx, dxsum, workspace, (hipStream_t)stream)
                      : ln_bwd_launch<float>(dy, lddy, x, ldx, rows, S, Cseg, gamma, mean, rstd, dx, lddx, dgamma, dbeta, M, accumulate_dx, dxsum, workspace, (hipStream_t)stream);
  if (rc) return rc;
  STSWIN_CHECK_LAUNCH();
  return 0;
}

/* dx = add + LN'(dy): the residual sum of a pre-norm block's backward written to a NEW buffer, so that `add` (the gradient of the block's
 * output branch, an operand of a weight-gradient GEMM that is launched later: stswin_gemm_tn_group) stays intact */
extern "C" int stswin_layernorm_bwd_add(int dtype, const void* dy, long lddy, const void* x, long ldx, const int* rows, int S,
                                        int Cseg, const float* gamma, const float* mean, const float* rstd, const void* add, long ldadd,
                                        void* dx, long lddx, float* dgamma, float* dbeta, int M, float* dxsum, float* workspace,
                                        void* stream) {
  const int pack = dtype == 0 ? 8 : 4;
  if (!add || Cseg % pack || ldx % pack || lddy % pack || lddx % pack || ldadd % pack) return -1105;
  if ((long)S * Cseg * 5 * 4 > 65536) return -1106;
  int rc = dtype == 0 ? ln_bwd_launch<bf16>(dy, lddy, x, ldx, rows, S, Cseg, gamma, mean, rstd, dx, lddx, dgamma, dbeta, M, 1, dxsum, workspace, (hipStream_t)stream, add, ldadd)
                      : ln_bwd_launch<float>(dy, lddy, x, ldx, rows, S, Cseg, gamma, mean, rstd, dx, lddx, dgamma, dbeta, M, 1, dxsum, workspace, (hipStream_t)stream, add, ldadd);
  if (rc) return rc;
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" long stswin_colsum_scratch(int M, int N) { return (long)((M + 511) / 512) * N; }
extern "C" int stswin_colsum(int dtype, const void* y, long ldy, float* out, int M, int N, float* scratch, void* stream) {
  const int pack = dtype == 0 ? 8 : 4;
  if (N % pack || ldy % pack) return -1107;
  if (!scratch) return -1111;
  if (M <= 0) return 0;
  const int rpb = 512;
  dim3 grid((N / pack + 31) / 32, (M + rpb - 1) / rpb);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(colsum_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)y, ldy, scratch, M, N, rpb);
  else
    hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(256), 0, st, (const float*)y, ldy, scratch, M, N, rpb);
  const int rc = stswin_fold_launch(scratch, N, 0, (int)grid.y, N, 1, out, nullptr, nullptr, 0, 1, 1, st);
  if (rc) return rc;
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_slab_fold(const float* ws, long slab_stride, long ws_batch_stride, int nslabs, int seg_len, int nseg, float* out0,
                                float* out1, float* out2, long out_batch_stride, int batch, int accumulate, void* stream) {
  const int rc = stswin_fold_launch(ws, slab_stride, ws_batch_stride, nslabs, seg_len, nseg, out0, out1, out2, out_batch_stride, batch,
                                    accumulate, (hipStream_t)stream);
  if (rc) return rc;
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_bias_expand(const float* table, const long* index, const float* mask, float* out, int N, int heads, int nW,
                                  void* stream) {
  if (N <= 0 || heads <= 0 || nW <= 0) return -1108;
  const long n = (long)nW * heads * N * N;
  hipLaunchKernelGGL(bias_expand_kernel, dim3((unsigned)min(2048L, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table,
                     index, mask, out, N, heads, nW);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_bias_expand_multi(int count, const float* const* table, const long* const* index, const float* const* mask,
                                        float* const* out, const int* N, const int* heads, const int* nW, void* stream) {
  if (count <= 0) return 0;
  if (count > BEM_MAX) return -1108;
  BiasExpandMulti a;
  long most = 0;
  for (int e = 0; e < BEM_MAX; ++e) {
    const int s = e < count ? e : 0;
    if (N[s] <= 0 || heads[s] <= 0 || nW[s] <= 0) return -1108;
    a.table[e] = table[s]; a.index[e] = index[s]; a.mask[e] = mask[s]; a.out[e] = out[s]; a.N[e] = N[s]; a.heads[e] = heads[s]; a.nW[e] = nW[s];
    const long n = (long)nW[s] * heads[s] * N[s] * N[s];
    if (n > most) most = n;
  }
  hipLaunchKernelGGL(bias_expand_multi_kernel, dim3((unsigned)min(256L, (most + 255) / 256), (unsigned)count), dim3(256), 0, (hipStream_t)stream, a);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_bias_scatter(const float* dbiasT, const int* order, const int* offs, float* dtable, int N, int heads, int table_rows,
                                   int nslabs, void* stream) {
  if (N <= 0 || heads <= 0 || table_rows <= 0 || nslabs <= 0 || !order || !offs) return -1109;
  hipLaunchKernelGGL(bias_scatter_kernel, dim3((unsigned)((table_rows * heads + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dbiasT,
                     order, offs, dtable, N, heads, table_rows, nslabs);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_vec_gather(const float* v, const int* map, float* out, int n, float fill, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(vec_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, v, map, out, n, fill);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_vec_gather_multi(int count, const float* const* v, const int* map, float* const* out, int n, const float* fill,
                                       void* stream) {
  if (n <= 0 || count <= 0) return 0;
  if (count > 4) return -1114;
  VecGatherMulti a;
  for (int k = 0; k < 4; ++k) { a.v[k] = k < count ? v[k] : nullptr; a.out[k] = k < count ? out[k] : nullptr; a.fill[k] = k < count ? fill[k] : 0.f; }
  a.map = map; a.n = n;
  hipLaunchKernelGGL(vec_gather_multi_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)count), dim3(256), 0, (hipStream_t)stream, a);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_linear_pack_multi(int dtype, int count, const float* const* w, void* const* fwd, void* const* tr, const int* n,
                                        const int* k, void* stream) {
  if (count <= 0) return 0;
  if (count > LPM_MAX) return -1113;
  LinearPackMulti a;
  long blocks = 0;
  for (int i = 0; i < count; ++i) {
    if (n[i] <= 0 || k[i] <= 0 || n[i] % 4 || k[i] % 4) return -1112;
    a.w[i] = w[i]; a.fwd[i] = fwd[i]; a.tr[i] = tr ? tr[i] : nullptr; a.n[i] = n[i]; a.k[i] = k[i];
    a.tiles[i] = ((k[i] + 63) / 64) * ((n[i] + 63) / 64);
    blocks += a.tiles[i];
  }
  a.count = count;
  if (dtype == 0) hipLaunchKernelGGL(linear_pack_multi_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(linear_pack_multi_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_conv_pack_multi(int dtype, int count, const float* const* w, void* const* fwd, void* const* dgrad,
                                      const int* const* omap, const int* const* imap, const int* ci, const int* S, const int* cop,
                                      const int* cip, void* stream) {
  if (count <= 0) return 0;
  if (count > CPM_MAX) return -1113;
  ConvPackMulti a;
  long blocks = 0;
  for (int i = 0; i < count; ++i) {
    if (ci[i] <= 0 || S[i] <= 0 || cop[i] <= 0 || cip[i] <= 0) return -1111;
    a.w[i] = w[i]; a.fwd[i] = fwd[i]; a.dg[i] = dgrad ? dgrad[i] : nullptr; a.omap[i] = omap[i]; a.imap[i] = imap[i];
    a.ci[i] = ci[i]; a.S[i] = S[i]; a.cop[i] = cop[i]; a.cip[i] = cip[i];
    a.tiles[i] = ((cip[i] + 63) / 64) * ((cop[i] + 63) / 64) * S[i];
    blocks += a.tiles[i];
  }
  a.count = count;
  if (dtype == 0) hipLaunchKernelGGL(conv_pack_multi_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(conv_pack_multi_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_linear_pack(int dtype, const float* w, void* fwd, void* tr, int n, int k, void* stream) {
  if (n <= 0 || k <= 0 || n % 4 || k % 4) return -1112;
  dim3 grid((unsigned)((k + 63) / 64), (unsigned)((n + 63) / 64));
  if (dtype == 0) hipLaunchKernelGGL(linear_pack_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, w, (bf16*)fwd, (bf16*)tr, n, k);
  else hipLaunchKernelGGL(linear_pack_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, w, (float*)fwd, (float*)tr, n, k);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Video inference (stswincl_amd/video.py).
//
// Frame ingest: uint8 RGB frames [n][Hs][Ws][3] -> fp32 images [n][3][H][W], the per-frame transform of
// seg18/dataset/Endovis2018_new.py:125-127 + seg18/test.py:149 (PIL resize BILINEAR, astype(float) / 255., .float()).
// Pillow's resampler is separable: a horizontal pass (only when the width changes) into a uint8 intermediate, then a
// vertical pass (only when the height changes).  Per output index: taps [xmin, xmin + n) with int32 weights of 22 fraction
// bits (host tables, stswincl_amd/video.py), out = clip((2^21 + sum u * k) >> 22, 0, 255).  Integer arithmetic only: the
// result is bit-exact with Pillow.  The value -> fp32 map is a 256-entry table (float32(u / 255.) of the reference).
// ---------------------------------------------------------------------------------------------------
DEVI int pil_clip8(int ss) {
  ss >>= 22;
  return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// the tap loop of one pass for the three channels of a pixel: s_c = 2^21 + sum_x src[x * step + c] * k[x * kstep], x < nk (src: the
// first tap's pixel, step: bytes between two taps).  Every resampling kernel of this file accumulates through it.
DEVI void pil_taps3(const unsigned char* src, long step, const int* k, int kstep, int nk, int& s0, int& s1, int& s2) {
  s0 = s1 = s2 = 1 << 21;
  for (int x = 0; x < nk; ++x) {
    const unsigned char* s = src + x * step;
    const int w = k[x * kstep];
    s0 += (int)s[0] * w;
    s1 += (int)s[1] * w;
    s2 += (int)s[2] * w;
  }
}

DEVI void pil_store3(unsigned char* dst, int s0, int s1, int s2) {
  dst[0] = (unsigned char)pil_clip8(s0);
  dst[1] = (unsigned char)pil_clip8(s1);
  dst[2] = (unsigned char)pil_clip8(s2);
}

// one thread per output pixel (row, xx) of the horizontal pass, three channels
__global__ __launch_bounds__(256) void ingest_hpass_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                            const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                            long rows, int Ws, int W) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * W) return;
  const long row = i / W;
  const int xx = (int)(i - row * W);
  const int xmin = bounds[2 * xx], nk = bounds[2 * xx + 1];
  const int* k = coef + (long)xx * ksize;
  int s0, s1, s2;
  pil_taps3(in + (row * Ws + xmin) * 3, 3, k, 1, nk, s0, s1, s2);
  pil_store3(out + i * 3, s0, s1, s2);
}

// one thread per output pixel (frame, yy, x): the vertical pass (bounds == NULL: the height is unchanged, no pass) + the table
// conversion into three fp32 planes (channel c reads lut[c * lut_stride + v]: stride 0 = one table for all three)
__global__ __launch_bounds__(256) void ingest_vpass_kernel(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                            const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                            const float* __restrict__ lut, int lut_stride, int n, int Hs, int H,
                                                            int W) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long plane = (long)H * W;
  if (i >= (long)n * plane) return;
  const int f = (int)(i / plane);
  const long p = i - (long)f * plane;
  const int yy = (int)(p / W), x = (int)(p - (long)yy * W);
  const unsigned char* src = in + (long)f * Hs * W * 3;
  int v0, v1, v2;
  if (bounds == nullptr) {
    const unsigned char* s = src + ((long)yy * W + x) * 3;
    v0 = s[0]; v1 = s[1]; v2 = s[2];
  } else {
    const int ymin = bounds[2 * yy], nk = bounds[2 * yy + 1];
    const int* k = coef + (long)yy * ksize;
    int s0, s1, s2;
    pil_taps3(src + ((long)ymin * W + x) * 3, (long)W * 3, k, 1, nk, s0, s1, s2);
    v0 = pil_clip8(s0); v1 = pil_clip8(s1); v2 = pil_clip8(s2);
  }
  float* o = out + (long)f * 3 * plane + p;
  o[0] = lut[v0];
  o[plane] = lut[lut_stride + v1];
  o[2 * plane] = lut[2 * lut_stride + v2];
}

static int frame_ingest_impl(const unsigned char* in, unsigned char* tmp, float* out, int n, int Hs, int Ws, int H, int W,
                             const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef, int vksize,
                             const float* lut, int lut_stride, void* stream) {
  if (n <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return -1801;
  if (in == nullptr || out == nullptr || lut == nullptr) return -1802;
  const bool hpass = Ws != W, vpass = Hs != H;
  if (hpass && (tmp == nullptr || hbounds == nullptr || hcoef == nullptr || hksize <= 0)) return -1803;
  if (vpass && (vbounds == nullptr || vcoef == nullptr || vksize <= 0)) return -1804;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* vin = in;
  if (hpass) {
    const long total = (long)n * Hs * W;
    hipLaunchKernelGGL(ingest_hpass_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, tmp, hbounds, hcoef, hksize,
                       (long)n * Hs, Ws, W);
    STSWIN_CHECK_LAUNCH();
    vin = tmp;
  }
  const long total = (long)n * H * W;
  hipLaunchKernelGGL(ingest_vpass_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, vin, out,
                     vpass ? vbounds : nullptr, vcoef, vksize, lut, lut_stride, n, Hs, H, W);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

extern "C" int stswin_frame_ingest(const unsigned char* in, unsigned char* tmp, float* out, int n, int Hs, int Ws, int H, int W,
                                   const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef,
                                   int vksize, const float* lut, void* stream) {
  return frame_ingest_impl(in, tmp, out, n, Hs, Ws, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, lut, 0, stream);
}

// The same with one table per RGB plane, lut [3][256] (segcata/dataset/CATA_new_512.py:228-229: (u / 255. - MEAN[c]) / STD[c]).
extern "C" int stswin_frame_ingest_planes(const unsigned char* in, unsigned char* tmp, float* out, int n, int Hs, int Ws, int H, int W,
                                          const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef,
                                          int vksize, const float* lut, void* stream) {
  return frame_ingest_impl(in, tmp, out, n, Hs, Ws, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, lut, 256, stream);
}

// Clip assembly from a frame-feature ring: unit u < B*4 writes clip frame u (= clip u / 4, position u % 4) from
// table[u] >= 0 -> ring slot table[u], table[u] < 0 -> fresh frame -1 - table[u]; unit B*4 + j stores fresh frame j into ring slot
// table[B*4 + j] (< 0: not kept).  Entries out of range write zeros / store nothing.  The caller guarantees that no slot a launch
// reads is one it stores into.  grid (pieces / 1024 rounded up, units), 16-byte pieces.
__global__ __launch_bounds__(256) void clip_assemble_kernel(uint4* ring, const uint4* fresh, uint4* clips, const int* table, int units,
                                                             int clip_units, int slots, int n_fresh, long pieces) {
  const int u = blockIdx.y;
  const int e = table[u];
  const uint4* src;
  uint4* dst;
  if (u < clip_units) {
    dst = clips + (long)u * pieces;
    src = e >= 0 ? (e < slots ? ring + (long)e * pieces : nullptr) : (-1 - e < n_fresh ? fresh + (long)(-1 - e) * pieces : nullptr);
  } else {
    const int j = u - clip_units;
    if (e < 0 || e >= slots || j >= n_fresh) return;
    dst = ring + (long)e * pieces;
    src = fresh + (long)j * pieces;
  }
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < pieces; c += (long)gridDim.x * 256)
    dst[c] = src != nullptr ? src[c] : make_uint4(0u, 0u, 0u, 0u);
}

extern "C" int stswin_clip_assemble(int dtype, void* ring, const void* fresh, void* clips, const int* table, int B, int n_store,
                                    int slots, int n_fresh, long frame_elems, void* stream) {
  if (B < 0 || n_store < 0 || B + n_store == 0 || slots < 0 || n_fresh < 0 || frame_elems <= 0) return -1805;
  const long bytes = frame_elems * (dtype == 0 ? 2 : 4);
  if (bytes % 16) return -1806;
  if (table == nullptr || (B > 0 && clips == nullptr) || (slots > 0 && ring == nullptr) || (n_fresh > 0 && fresh == nullptr))
    return -1807;
  const long pieces = bytes / 16;
  const int units = B * 4 + n_store;
  const long gx = (pieces + 1023) / 1024;
  hipLaunchKernelGGL(clip_assemble_kernel, dim3((unsigned)(gx < 64 ? gx : 64), (unsigned)units), dim3(256), 0, (hipStream_t)stream,
                     (uint4*)ring, (const uint4*)fresh, (uint4*)clips, table, units, B * 4, slots, n_fresh, pieces);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Training input (stswincl_amd/augment.py): the transform of seg18/dataset/Endovis2018_new.py:61-107, 145-182 on uint8 clips and
// labels, in two stages.  Integer arithmetic only until the last table lookup; everything a sample needs that is not a pixel comes
// from its row of a host-made int32 table (layouts in include/stswin_hip.h).  Table values that would leave a source are clamped:
// a wrong table gives wrong pixels, never a wild read.
//
// Stage 1, scale + pad + crop + flip: Pillow's BILINEAR as the ingest kernels above compute it, for the crop window only.  The
// horizontal pass writes the window's columns of the source rows [r0, r1) that the window's rows read into the uint8 intermediate
// tmp [B][T][Hs][Wc][3]; the vertical pass writes the crop [B][T][Hc][Wc][3] at the flipped address.  A padded column or row has
// no taps and comes out as (2^21) >> 22 = 0, ImageOps.expand(fill=0).  The label takes Pillow's NEAREST source index per column /
// row (< 0: padding, label 0).
// ---------------------------------------------------------------------------------------------------
#define AUG1_HEAD 4      // r0, r1, flags (1 = horizontal flip, 2 = vertical flip), 0
#define AUG2_HEAD 4      // flags (1 = rotate), then key0, key1, noise: read by augment_noise_kernel only

// grid (Hs * Wc / 256, B * T): one thread per (source row, window column) of a frame
__global__ __launch_bounds__(256) void augment_hpass_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ tmp,
                                                             const int* __restrict__ table, long tstride, int ksize, int T, int Hs,
                                                             int Ws, int Wc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Hs * Wc) return;
  const int f = blockIdx.y;
  const int* tab = table + (long)(f / T) * tstride;
  const int row = i / Wc, j = i - row * Wc;
  if (row < tab[0] || row >= tab[1]) return;
  int xmin = tab[AUG1_HEAD + 2 * j], nk = tab[AUG1_HEAD + 2 * j + 1];
  xmin = xmin < 0 ? 0 : (xmin > Ws ? Ws : xmin);
  nk = nk > ksize ? ksize : nk;
  nk = nk > Ws - xmin ? Ws - xmin : nk;
  const int* k = tab + AUG1_HEAD + 2 * Wc + (long)j * ksize;
  int s0, s1, s2;
  pil_taps3(in + (((long)f * Hs + row) * Ws + xmin) * 3, 3, k, 1, nk, s0, s1, s2);
  pil_store3(tmp + (((long)f * Hs + row) * Wc + j) * 3, s0, s1, s2);
}

// grid (Hc * Wc / 256, B * T): one thread per crop pixel of a frame; a sample's first frame also writes its label crop
__global__ __launch_bounds__(256) void augment_vpass_kernel(const unsigned char* __restrict__ tmp, const unsigned char* __restrict__ labels,
                                                             unsigned char* __restrict__ crop, unsigned char* __restrict__ label_crop,
                                                             const int* __restrict__ table, long tstride, int ksize, int T, int Hs,
                                                             int Ws, int Hc, int Wc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Hc * Wc) return;
  const int f = blockIdx.y, b = f / T;
  const int* tab = table + (long)b * tstride;
  const int y = i / Wc, x = i - y * Wc;
  const int* vb = tab + AUG1_HEAD + (2 + ksize) * Wc;
  int ymin = vb[2 * y], nk = vb[2 * y + 1];
  ymin = ymin < 0 ? 0 : (ymin > Hs ? Hs : ymin);
  nk = nk > ksize ? ksize : nk;
  nk = nk > Hs - ymin ? Hs - ymin : nk;
  const int* k = vb + 2 * Hc + (long)y * ksize;
  int s0, s1, s2;
  pil_taps3(tmp + (((long)f * Hs + ymin) * Wc + x) * 3, (long)Wc * 3, k, 1, nk, s0, s1, s2);
  const int flags = tab[2];
  const int xo = (flags & 1) ? Wc - 1 - x : x, yo = (flags & 2) ? Hc - 1 - y : y;
  pil_store3(crop + (((long)f * Hc + yo) * Wc + xo) * 3, s0, s1, s2);
  if (f - b * T == 0) {
    const int* lx = vb + (2 + ksize) * Hc;
    const int sx = lx[x], sy = lx[Wc + y];
    const bool inside = sx >= 0 && sx < Ws && sy >= 0 && sy < Hs;
    label_crop[((long)b * Hc + yo) * Wc + xo] = inside ? labels[((long)b * Hs + sy) * Ws + sx] : (unsigned char)0;
  }
}

extern "C" long stswin_augment_crop_table_stride(int Hc, int Wc, int ksize) {
  return AUG1_HEAD + (long)(2 + ksize) * (Hc + Wc) + Hc + Wc;
}

extern "C" int stswin_augment_crop(const unsigned char* frames, const unsigned char* labels, unsigned char* tmp, unsigned char* crop,
                                   unsigned char* label_crop, const int* table, long table_stride, int ksize, int B, int T, int Hs,
                                   int Ws, int Hc, int Wc, void* stream) {
  if (B <= 0 || T <= 0 || Hs <= 0 || Ws <= 0 || Hc <= 0 || Wc <= 0 || ksize <= 0) return -1811;
  if (frames == nullptr || labels == nullptr || tmp == nullptr || crop == nullptr || label_crop == nullptr || table == nullptr)
    return -1812;
  if (table_stride < stswin_augment_crop_table_stride(Hc, Wc, ksize)) return -1813;
  if ((long)Hs * Wc > (1L << 30) || (long)Hc * Wc > (1L << 30) || (long)B * T > 65535) return -1814;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(augment_hpass_kernel, dim3((unsigned)((Hs * Wc + 255) / 256), (unsigned)(B * T)), dim3(256), 0, st, frames, tmp,
                     table, table_stride, ksize, T, Hs, Ws, Wc);
  STSWIN_CHECK_LAUNCH();
  hipLaunchKernelGGL(augment_vpass_kernel, dim3((unsigned)((Hc * Wc + 255) / 256), (unsigned)(B * T)), dim3(256), 0, st, tmp, labels,
                     crop, label_crop, table, table_stride, ksize, T, Hs, Ws, Hc, Wc);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Stage 2, value table + rotate + convert.  The sample's uint8 -> uint8 table (brightness / contrast; identity when unused) is
// applied to every source pixel BEFORE the interpolation, the reference's order.  Rotation: the source position of output (y, x)
// in 1/32 pixel is ((rowx[y] + colx[x]) >> 5, (rowy[y] + coly[x]) >> 5) from the host's 10-bit tables (the rounding term is in
// the row tables); weights (32 - fx | fx) x (32 - fy | fy), out = (sum w v + 512) >> 10, reflect-101 border; the label takes the
// nearest source pixel ((X + 16) >> 5, (Y + 16) >> 5).  A sample without rotation copies through.  Then byte -> fp32 through
// lut[c * lut_stride + v] into planes, label -> int64 through label_lut[256].
DEVI int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  i %= period;
  if (i < 0) i += period;
  return i >= n ? period - i : i;
}

// grid (Hc * Wc / 256, B): one thread per output pixel of a sample, all T frames and the label
__global__ __launch_bounds__(256) void augment_finish_kernel(const unsigned char* __restrict__ crop, const unsigned char* __restrict__ label_crop,
                                                              float* __restrict__ images, long* __restrict__ labels_out,
                                                              const int* __restrict__ table, long tstride, const float* __restrict__ lut,
                                                              int lut_stride, const long* __restrict__ label_lut, int T, int Hc, int Wc) {
  __shared__ int bc_words[64];
  const int b = blockIdx.y;
  const int* tab = table + (long)b * tstride;
  if (threadIdx.x < 64) bc_words[threadIdx.x] = tab[AUG2_HEAD + 2 * (Wc + Hc) + threadIdx.x];
  __syncthreads();
  const unsigned char* bc = (const unsigned char*)bc_words;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int plane = Hc * Wc;
  if (p >= plane) return;
  const int y = p / Wc, x = p - y * Wc;
  const unsigned char* lab = label_crop + (long)b * plane;
  if (!(tab[0] & 1)) {
    for (int t = 0; t < T; ++t) {
      const unsigned char* s = crop + (((long)b * T + t) * plane + p) * 3;
      float* o = images + ((long)b * T + t) * 3 * plane + p;
      o[0] = lut[bc[s[0]]];
      o[plane] = lut[lut_stride + bc[s[1]]];
      o[2 * (long)plane] = lut[2 * lut_stride + bc[s[2]]];
    }
    labels_out[(long)b * plane + p] = label_lut[lab[p]];
    return;
  }
  const int* colx = tab + AUG2_HEAD;
  const int* rowx = colx + 2 * Wc;
  const int X = (rowx[y] + colx[x]) >> 5, Y = (rowx[Hc + y] + colx[Wc + x]) >> 5;
  const int fx = X & 31, fy = Y & 31;
  const int x0 = reflect101(X >> 5, Wc), x1 = reflect101((X >> 5) + 1, Wc);
  const int y0 = reflect101(Y >> 5, Hc), y1 = reflect101((Y >> 5) + 1, Hc);
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
  const int o00 = (y0 * Wc + x0) * 3, o01 = (y0 * Wc + x1) * 3, o10 = (y1 * Wc + x0) * 3, o11 = (y1 * Wc + x1) * 3;
  for (int t = 0; t < T; ++t) {
    const unsigned char* s = crop + ((long)b * T + t) * plane * 3;
    float* o = images + ((long)b * T + t) * 3 * plane + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = (w00 * bc[s[o00 + c]] + w01 * bc[s[o01 + c]] + w10 * bc[s[o10 + c]] + w11 * bc[s[o11 + c]] + 512) >> 10;
      o[(long)c * plane] = lut[c * lut_stride + v];
    }
  }
  const int nx = reflect101((X + 16) >> 5, Wc), ny = reflect101((Y + 16) >> 5, Hc);
  labels_out[(long)b * plane + p] = label_lut[lab[ny * Wc + nx]];
}

extern "C" long stswin_augment_finish_table_stride(int Hc, int Wc) { return AUG2_HEAD + 2L * (Hc + Wc) + 64; }

extern "C" int stswin_augment_finish(const unsigned char* crop, const unsigned char* label_crop, float* images, long* labels_out,
                                     const int* table, long table_stride, const float* lut, int lut_planes, const long* label_lut,
                                     int B, int T, int Hc, int Wc, void* stream) {
  if (B <= 0 || T <= 0 || Hc <= 0 || Wc <= 0) return -1815;
  if (crop == nullptr || label_crop == nullptr || images == nullptr || labels_out == nullptr || table == nullptr || lut == nullptr ||
      label_lut == nullptr)
    return -1816;
  if (table_stride < stswin_augment_finish_table_stride(Hc, Wc)) return -1817;
  if ((long)Hc * Wc > (1L << 28) || B > 65535) return -1818;
  hipLaunchKernelGGL(augment_finish_kernel, dim3((unsigned)((Hc * Wc + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     crop, label_crop, images, labels_out, table, table_stride, lut, lut_planes ? 256 : 0, label_lut, T, Hc, Wc);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// Between the stages, CaDIS's Gaussian noise (segcata/dataset/CATA_new_512.py:178-183) in place on stage 1's uint8 crop.  The
// reference stores (255 * clip(u / 255. + n, 0, 1)).astype('uint8') = clamp(u + floor(255 n), 0, 255): an integer offset K with a
// fixed discrete law, which the host states as ascending 32-bit thresholds (K = k_min + the number of thresholds <= r for a uniform
// 32-bit r).  r comes from Philox4x32-10 (Salmon et al., Random123) keyed by the sample's 64-bit key from words 1, 2 of its stage-2
// table row and counted by the byte index: bytes 4c .. 4c + 3 of a sample take the four words of counter (c, 0, 0, 0).  A byte's
// noise is therefore a function of (key, byte index) alone: launch geometry, alignment and the path taken do not enter.
DEVI void philox4x32_10(unsigned c0, unsigned k0, unsigned k1, unsigned (&w)[4]) {
  unsigned c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

#define AUGN_MAX_THR 1024
#define AUGN_MIN_STRIDE (AUG2_HEAD + 2L * (1 + 1) + 64)      // stswin_augment_finish_table_stride(1, 1): the shortest stage-2 row

// #{j < n : thr[j] < v}, thr ascending
DEVI int augn_count_below(const unsigned* thr, int n, unsigned v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// clamp(u + k_min + #{j : thr[j] <= r}, 0, 255).  guide[t] = #{j : thr[j] < t << 24} (guide[256] = n), so the top byte of r
// brackets the count (most brackets hold no or one threshold; the tails of the law, dense near 0 and 2^32, fall into the first and
// the last); a binary search inside the bracket finishes.  Indices stay inside [0, n) whatever the thresholds hold.
DEVI unsigned augn_byte(unsigned u, unsigned r, const unsigned* thr, const unsigned short* guide, int k_min) {
  int lo = guide[r >> 24], hi = guide[(r >> 24) + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= r) lo = mid + 1; else hi = mid;
  }
  const int v = (int)u + k_min + lo;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one 4-byte unit, bytes in memory order (little endian), of counter `unit`
DEVI unsigned augn_word(unsigned word, unsigned unit, unsigned k0, unsigned k1, const unsigned* thr, const unsigned short* guide,
                        int k_min) {
  unsigned w[4];
  philox4x32_10(unit, k0, k1, w);
  unsigned out = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) out |= augn_byte((word >> (8 * j)) & 0xffu, w[j], thr, guide, k_min) << (8 * j);
  return out;
}

// grid (blocks per sample, samples): a sample with noise == 0 is left alone.  A sample is `units` 4-byte units.  Those from the
// first 16-byte aligned address on go four at a time through 16-byte loads and stores (the wide body); the `head` units in front
// of it and the < 4 behind it, or every unit of a sample whose base is not 4-byte aligned, go byte by byte (the narrow body).
__global__ __launch_bounds__(256) void augment_noise_kernel(unsigned char* __restrict__ crop, const int* __restrict__ table, long tstride,
                                                             const unsigned* __restrict__ thr_in, int n_thr, int k_min, int B,
                                                             long sample_bytes) {
  __shared__ unsigned thr[AUGN_MAX_THR];
  __shared__ unsigned short guide[258];
  for (int j = threadIdx.x; j < n_thr; j += 256) thr[j] = thr_in[j];
  __syncthreads();
  for (int t = threadIdx.x; t <= 256; t += 256)
    guide[t] = (unsigned short)(t == 256 ? n_thr : augn_count_below(thr, n_thr, (unsigned)t << 24));
  __syncthreads();
  const long units = sample_bytes >> 2;
  const long first = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int* tab = table + (long)b * tstride;
    if (tab[3] == 0) continue;
    const unsigned k0 = (unsigned)tab[1], k1 = (unsigned)tab[2];
    unsigned char* base = crop + (long)b * sample_bytes;
    const unsigned long addr = (unsigned long)base;
    long head = (addr & 3ul) ? units : (long)(((16ul - (addr & 15ul)) & 15ul) >> 2);
    head = head > units ? units : head;
    const long nwide = (units - head) >> 2, tail = units - head - 4 * nwide;
    uint4* wide = (uint4*)(base + 4 * head);
    for (long i = first; i < nwide; i += step) {
      uint4 v = wide[i];
      const unsigned unit = (unsigned)(head + 4 * i);
      v.x = augn_word(v.x, unit, k0, k1, thr, guide, k_min);
      v.y = augn_word(v.y, unit + 1u, k0, k1, thr, guide, k_min);
      v.z = augn_word(v.z, unit + 2u, k0, k1, thr, guide, k_min);
      v.w = augn_word(v.w, unit + 3u, k0, k1, thr, guide, k_min);
      wide[i] = v;
    }
    for (long i = first; i < head + tail; i += step) {
      const long unit = i < head ? i : i + 4 * nwide;
      unsigned char* p = base + 4 * unit;
      const unsigned word = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
      const unsigned out = augn_word(word, (unsigned)unit, k0, k1, thr, guide, k_min);
      p[0] = (unsigned char)out, p[1] = (unsigned char)(out >> 8), p[2] = (unsigned char)(out >> 16), p[3] = (unsigned char)(out >> 24);
    }
  }
}

extern "C" int stswin_augment_noise(unsigned char* crop, const int* table, long table_stride, const unsigned int* thr, int n_thr,
                                    int k_min, int B, long sample_bytes, void* stream) {
  if (B <= 0 || sample_bytes <= 0 || (sample_bytes & 3) || sample_bytes > (1L << 34)) return -1808;
  if (crop == nullptr || table == nullptr || thr == nullptr) return -1809;
  if (n_thr < 1 || n_thr > AUGN_MAX_THR) return -1810;
  if (table_stride < AUGN_MIN_STRIDE) return -1819;
  k_min = k_min < -2048 ? -2048 : (k_min > 2048 ? 2048 : k_min);      // (beyond +-(255 + 1024) every byte clamps the same way)
  // a thread per 16-byte piece of a sample: the pass is bound by its dependent LDS reads, not by memory, and more waves hide more
  // of them than longer threads save in table set-up (31.5 MB in 4 samples: 26 us so against 32 us at four pieces per thread)
  long gx = (((sample_bytes + 15) >> 4) + 255) >> 8;
  gx = gx > 4096 ? 4096 : gx;
  hipLaunchKernelGGL(augment_noise_kernel, dim3((unsigned)gx, (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, (hipStream_t)stream, crop,
                     table, table_stride, thr, n_thr, k_min, B, sample_bytes);
  STSWIN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Contrastive pre-training input (stswincl_amd/contrast/views.py): the six RandomResizedCropCoord + RandomHorizontalFlipCoord +
// ToTensor + Normalize pipelines of pixcontrast_18/contrast/data/dataset.py:43-70 on the uint8 frames and labels as they are
// stored.  One table row per output view-sample names its four source frames and its label, so views that share frames read them
// in place; the crop + resize is the resampler above for the crop's taps, and the vertical pass writes the fp32 planes and the
// fp32 mask itself: no uint8 crop goes through memory.  Every index a table supplies is clamped into its source: a wrong table
// gives wrong pixels, never a wild read.
// ---------------------------------------------------------------------------------------------------
#define CV_HEAD 8        // r0, r1, flags (1 = horizontal flip, 2 = vertical flip), label index, four frame indices
#define CV_MAX_KSIZE 16
#define CV_HROWS 8       // source rows per block of the horizontal pass

DEVI int cv_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// grid (W / 256, Hs / CV_HROWS, V * 4): a block takes 256 output columns of CV_HROWS source rows of one frame of a view.  The
// columns' weights go through LDS once per block ([tap][column]: conflict-free for any ksize); the rows outside [r0, r1) - a
// block-uniform test - are not computed.
__global__ __launch_bounds__(256) void contrast_views_hpass_kernel(const unsigned char* __restrict__ frames, unsigned char* __restrict__ tmp,
                                                                    const int* __restrict__ table, long tstride, int ksize, int F,
                                                                    int Hs, int Ws, int W) {
  __shared__ int sk[CV_MAX_KSIZE * 256];
  const int u = blockIdx.z;
  const int* tab = table + (long)(u >> 2) * tstride;
  int ra = blockIdx.y * CV_HROWS, rb = ra + CV_HROWS;
  const int r0 = tab[0] < 0 ? 0 : tab[0], r1 = tab[1] > Hs ? Hs : tab[1];
  ra = ra < r0 ? r0 : ra;
  rb = rb > r1 ? r1 : rb;
  if (ra >= rb) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= W) return;
  int xmin = tab[CV_HEAD + 2 * j], nk = tab[CV_HEAD + 2 * j + 1];
  xmin = xmin < 0 ? 0 : (xmin > Ws ? Ws : xmin);
  nk = nk > ksize ? ksize : nk;
  nk = nk > Ws - xmin ? Ws - xmin : nk;
  const int* k = tab + CV_HEAD + 2 * W + (long)j * ksize;
  for (int x = 0; x < nk; ++x) sk[x * 256 + threadIdx.x] = k[x];          // (a thread reads only the words it wrote itself: no barrier)
  const int f = cv_clamp(tab[4 + (u & 3)], F);
  const unsigned char* src = frames + ((long)f * Hs * Ws + xmin) * 3;
  unsigned char* dst = tmp + ((long)u * Hs * W + j) * 3;
  for (int row = ra; row < rb; ++row) {
    int s0, s1, s2;
    pil_taps3(src + (long)row * Ws * 3, 3, sk + threadIdx.x, 256, nk, s0, s1, s2);
    pil_store3(dst + (long)row * W * 3, s0, s1, s2);
  }
}

// grid (W / 256, H, V * 4): a block takes 256 columns of one output row of one frame of a view, so the row's taps and weights are
// block-uniform (scalar loads, no per-thread table reads); it stores the three fp32 planes at the flipped address, and the view's
// first frame also stores the mask.
__global__ __launch_bounds__(256) void contrast_views_vpass_kernel(const unsigned char* __restrict__ tmp, const unsigned char* __restrict__ labels,
                                                                    float* __restrict__ images, float* __restrict__ masks,
                                                                    const int* __restrict__ table, long tstride, const float* __restrict__ lut,
                                                                    int ksize, int L, int Hs, int Ws, int H, int W) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  const int y = blockIdx.y, u = blockIdx.z, v = u >> 2;
  const int* tab = table + (long)v * tstride;
  const int* vb = tab + CV_HEAD + (long)(2 + ksize) * W;
  int ymin = vb[2 * y], nk = vb[2 * y + 1];
  ymin = ymin < 0 ? 0 : (ymin > Hs ? Hs : ymin);
  nk = nk > ksize ? ksize : nk;
  nk = nk > Hs - ymin ? Hs - ymin : nk;
  int s0, s1, s2;
  pil_taps3(tmp + (((long)u * Hs + ymin) * W + x) * 3, (long)W * 3, vb + 2 * H + (long)y * ksize, 1, nk, s0, s1, s2);
  const int flags = tab[2];
  const int xo = (flags & 1) ? W - 1 - x : x, yo = (flags & 2) ? H - 1 - y : y;
  const long plane = (long)H * W, p = (long)yo * W + xo;
  float* o = images + (long)u * 3 * plane + p;
  o[0] = lut[pil_clip8(s0)];
  o[plane] = lut[256 + pil_clip8(s1)];
  o[2 * plane] = lut[512 + pil_clip8(s2)];
  if ((u & 3) == 0) {
    const int* lx = vb + (long)(2 + ksize) * H;
    const int sx = cv_clamp(lx[x], Ws), sy = cv_clamp(lx[W + y], Hs), l = cv_clamp(tab[3], L);
    masks[(long)v * plane + p] = (float)labels[((long)l * Hs + sy) * Ws + sx];
  }
}

extern "C" long stswin_contrast_views_table_stride(int H, int W, int ksize) {
  return CV_HEAD + (long)(2 + ksize) * (H + W) + H + W;
}

extern "C" int stswin_contrast_views(const unsigned char* frames, const unsigned char* labels, unsigned char* tmp, float* images,
                                     float* masks, const int* table, long table_stride, const float* lut, int ksize, int V, int F,
                                     int L, int Hs, int Ws, int H, int W, void* stream) {
  if (V <= 0 || F <= 0 || L <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || ksize <= 0) return -1821;
  if (frames == nullptr || labels == nullptr || tmp == nullptr || images == nullptr || masks == nullptr || table == nullptr ||
      lut == nullptr)
    return -1822;
  if (ksize > CV_MAX_KSIZE) return -1823;
  if (table_stride < stswin_contrast_views_table_stride(H, W, ksize)) return -1824;
  if ((long)V * 4 > 65535 || H > 65535 || (long)Hs > 65535L * CV_HROWS || (long)Hs * Ws > (1L << 28) || (long)H * W > (1L << 28))
    return -1825;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)((W + 255) / 256);
  hipLaunchKernelGGL(contrast_views_hpass_kernel, dim3(gx, (unsigned)((Hs + CV_HROWS - 1) / CV_HROWS), (unsigned)(V * 4)), dim3(256), 0,
                     st, frames, tmp, table, table_stride, ksize, F, Hs, Ws, W);
  STSWIN_CHECK_LAUNCH();
  hipLaunchKernelGGL(contrast_views_vpass_kernel, dim3(gx, (unsigned)H, (unsigned)(V * 4)), dim3(256), 0, st, tmp, labels, images, masks,
                     table, table_stride, lut, ksize, L, Hs, Ws, H, W);
  STSWIN_CHECK_LAUNCH();
  return 0;
}
