"""Float64 reference of the four kernels of stswincl_amd/csrc/conv_halo.hip (stswin_conv3x3_c64, stswin_conv3x3_c64_wgrad,
stswin_stem_conv, stswin_stem_wgrad), the launcher's schedules, derived PER-ELEMENT error bounds and the case list of the contract tests.

Shared by tests/test_conv_halo_ref.py (CPU: the reference against float64 torch convolutions, the schedules against the launcher's
expressions, every case's recorded properties, the bounds against an fp32 emulation and against nine planted defects) and
tests/test_hip_conv_halo_contract.py (GPU: every kernel against it).  Nothing here calls the library: plain torch in float64 on the
operands the kernels multiply (bf16 tensors cast to float64), on whatever device the operands live.

Contracts (include/stswin_hip.h), each computed as a sum of shifted matmuls so that A = sum |x * w| comes out of the same code:
  conv3x3_c64        y[p][co] = sum_{tap, ci} x[p + sign * off(tap)][ci] * wmat[co][tap * 64 + ci]  (+ resid[p][co])
                     tap = ky * 3 + kx, off(tap) = (ky - 1, kx - 1); zeros outside the frame in both directions, frames never bleed into
                     each other.  wmat: fwd [cout][tap][cin] with sign = +1, dgrad [cin][tap][cout] with sign = -1, taps in forward order.
  conv3x3_c64_wgrad  dW[co][tap][ci] = sum_p dy[p][co] * x[p + off(tap)][ci]; stored [co][tap][ci] or (tapminor) [co][ci][tap]; += c_prev.
  stem_conv          y[p][co] = sum_{s, t, ch} rec[(oy + s, ox + t)][ch] * W[co][s][t][ch]   over records [F][Ho + 3][Wo + 3][16]: a general
  stem_wgrad         dW[co][s][t][ch] = sum_p dy[p][co] * rec[(oy + s, ox + t)][ch]          4 x 4 convolution over 16-value records.
                     The contract tests feed a DENSE rec and a dense W (no structural zeros: an exchanged record / position index shows);
                     tests/test_conv_halo_ref.py ties the general form back to the 7 x 7 / 2 / 3 convolution.

Schedules (the launcher's rule, conv_halo.hip): fwd_schedule / wgrad_schedule / stem_schedule return every workgroup's run of tiles or
units.  A forward tile is 256 pixels, a weight-gradient unit 128 pixels, a stem unit one output row of a 128-wide strip.

Bounds: derived, nothing is measured on a GPU.  u = 2^-23 and the argument of tests/gemm_ref.py: any summation order, each operation
loses at most one ulp one-sidedly of a partial sum bounded by A, bf16 products are exact in fp32.
  outputs      E = (K + 2) * u * A with K = 576 (halo) or 256 (stem); the residual's one fp32 add: + u * (|ref| + E); the bf16 store:
               + half_ulp_bf16(|ref| + E').
  statistics   a table row holds the fp32 sum of the values BEFORE the store, and of their squares, over the rows the schedule gives it:
               sum of the per-element E' over those n rows + (n + 2) * u * sum (|v| + E'); squares: sum (2 |v| E' + E'^2) +
               (n + 3) * u * sum (|v| + E')^2 (one more operation per term: the square itself is rounded).
  gradients    gemm_tn_ref.bound() for fp32 slabs: per workgroup (rows_s + 2) * u * A_s, rows_s = per * 128, then the fixed-order fold
               over `grid` slabs and onto c_prev: (grid + 2) * u * (|c_prev| + sum_s (|P_s| + E_s)).
Operand flavours: 'signed' (standard normal operands: cancellation, so the accumulation term matters) and 'nonneg' (their absolute
values: A = |ref|, the tightest bound the formulas give relative to the result - only there can a statistics row tell the sum of the
pre-store values from the sum of the stored ones, see test_conv_halo_ref.py)."""
from __future__ import annotations

import dataclasses
from typing import NamedTuple

import torch
import torch.nn.functional as Fn

from gemm_ref import U, half_ulp_bf16
from gemm_tn_ref import bound as slab_bound, to_tapminor

F64 = torch.float64
BF = torch.bfloat16
TAPS = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ schedules
class Sched(NamedTuple):
    units: int          # tiles (forward) or units
    upf: int            # units per frame (halo kernels) or per strip (stem: Ho)
    per: int
    grid: int           # workgroups launched
    runs: list          # [(u0, u1)] per workgroup; u0 == u1: the workgroup returns at once

    def where(self, u):
        """-> (workgroup, position in its run) of unit u."""
        return u // self.per, u % self.per

    def stretches(self):
        """[(u0, u1)]: every run cut at the frame / strip changes inside it."""
        out = []
        for u0, u1 in self.runs:
            a = u0
            while a < u1:
                b = min(u1, (a // self.upf + 1) * self.upf)
                out.append((a, b))
                a = b
        return out

    def crossing(self):
        """Runs that hold units of more than one frame / strip."""
        return sum(1 for u0, u1 in self.runs if u1 > u0 and (u1 - 1) // self.upf != u0 // self.upf)


def _runs(units, per, grid):
    return [(min(units, b * per), min(units, (b + 1) * per)) for b in range(grid)]


def fwd_schedule(F, H, W):
    """stswin_conv3x3_c64: tiles of 256 pixels, min(tiles, 256) workgroups, per = ceil(tiles / grid) consecutive tiles each."""
    assert (H * W) % 256 == 0 and W in (16, 32, 64, 128)
    tiles = F * H * W // 256
    grid = min(tiles, 256)
    per = cdiv(tiles, grid)
    return Sched(tiles, H * W // 256, per, grid, _runs(tiles, per, grid))


def wgrad_schedule(F, H, W):
    """stswin_conv3x3_c64_wgrad: units of 128 pixels, per = ceil(units / min(units, 256)), ceil(units / per) workgroups (= slabs)."""
    assert (H * W) % 128 == 0 and W in (32, 64, 128)
    units = F * H * W // 128
    per = cdiv(units, min(units, 256))
    grid = cdiv(units, per)
    return Sched(units, H * W // 128, per, grid, _runs(units, per, grid))


def ring_slots(W):
    return {128: 4, 64: 8, 32: 16}[W]


def stem_geometry(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_schedule(F, H, W):
    """stswin_stem_conv / stswin_stem_wgrad over images [F][3][H][W]: unit u = output row u % Ho of strip u // Ho (strip = frame *
    (Wo / 128) + column block), the weight gradient's per / grid rule.  Sched.stretches() are the statistics runs of stem_conv."""
    Ho, Wo = stem_geometry(H, W)
    assert Wo % 128 == 0
    units = F * (Wo // 128) * Ho
    per = cdiv(units, min(units, 256))
    grid = cdiv(units, per)
    return Sched(units, Ho, per, grid, _runs(units, per, grid))


def stem_unit_pixels(F, H, W, device="cpu"):
    """long [units][128]: the output pixels (rows of y / dy) of every stem unit, in unit order."""
    Ho, Wo = stem_geometry(H, W)
    nxh = Wo // 128
    u = torch.arange(F * nxh * Ho, device=device)
    strip, oy = u // Ho, u % Ho
    f, xb = strip // nxh, strip % nxh
    pix0 = (f * Ho + oy) * Wo + xb * 128
    return pix0[:, None] + torch.arange(128, device=device)[None, :]


# ------------------------------------------------------------------------------------------------------------------ operands
def conv_wmats(w):
    """(64, 64, 3, 3) weight -> (fwd [cout][tap * 64 + cin], dgrad [cin][tap * 64 + cout]), the header's definition in torch."""
    co, ci = w.shape[:2]
    return w.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous(), w.permute(1, 2, 3, 0).reshape(ci, 9 * co).contiguous()


def shifted(X, dy, dx):
    """X [F][H][W][C] -> the same shape, pixel (y, x) holding X[y + dy][x + dx], zeros outside the frame."""
    H, W = X.shape[1:3]
    py, px = abs(dy), abs(dx)
    Xp = Fn.pad(X, (0, 0, px, px, py, py))
    return Xp[:, py + dy:py + dy + H, px + dx:px + dx + W]


def conv3x3_terms(x, wmat, F, H, W, sign):
    """-> (y0, A) float64 [F*H*W][64]: the convolution without residual and its sum of absolute products."""
    X = x.to(F64).view(F, H, W, 64)
    Wt = wmat.to(F64).t().contiguous()
    Wa = Wt.abs()
    step = max(1, 8192 // (H * W))                        # whole frames, ~8192 pixels at a time: the nine shifted copies side by side
    ys, As = [], []
    for f0 in range(0, F, step):
        B = torch.cat([shifted(X[f0:f0 + step], sign * dy, sign * dx).reshape(-1, 64) for dy, dx in TAPS], dim=1)
        ys.append(B @ Wt)
        As.append(B.abs_() @ Wa)
    return torch.cat(ys), torch.cat(As)


def stem_terms(rec, wmat, F, H, W):
    """rec: flat [F * (Ho+3) * (Wo+3) * 16 (+ trailing)], wmat [64][256] = [co][s][t][ch] -> (y0, A) float64 [F*Ho*Wo][64]."""
    Ho, Wo = stem_geometry(H, W)
    R = rec[:F * (Ho + 3) * (Wo + 3) * 16].to(F64).view(F, Ho + 3, Wo + 3, 16)
    Wd = wmat.to(F64).view(64, 4, 4, 16)
    y = torch.zeros(F * Ho * Wo, 64, dtype=F64, device=rec.device)
    A = torch.zeros_like(y)
    for s in range(4):
        for t in range(4):
            r = R[:, s:s + Ho, t:t + Wo].reshape(-1, 16)
            y += r @ Wd[:, s, t].t()
            A += r.abs() @ Wd[:, s, t].abs().t()
    return y, A


def _slab_products(DY, B, sched, rows_per_unit=128):
    """DY [M][64], B [M][n] in UNIT order -> (P, Ab) [grid][64][n]: every workgroup's partial DY^T B over its run."""
    M, n = B.shape
    rows = sched.per * rows_per_unit
    pad = sched.grid * rows - M
    DYp = Fn.pad(DY, (0, 0, 0, pad)).view(sched.grid, rows, 64).transpose(1, 2)
    Bp = Fn.pad(B, (0, 0, 0, pad)).view(sched.grid, rows, n)
    return torch.bmm(DYp, Bp), torch.bmm(DYp.abs(), Bp.abs())


def conv3x3_wgrad_partials(dy, x, F, H, W, sched):
    """-> (P, Ab) float64 [grid][64][576] in GEMM order [co][tap][ci]."""
    X = x.to(F64).view(F, H, W, 64)
    B = torch.cat([shifted(X, dy_, dx_).reshape(-1, 64) for dy_, dx_ in TAPS], dim=1)
    return _slab_products(dy.to(F64), B, sched)


def stem_wgrad_partials(dy, rec, F, H, W, sched):
    """-> (P, Ab) float64 [grid][64][256] = [co][s][t][ch]."""
    Ho, Wo = stem_geometry(H, W)
    R = rec[:F * (Ho + 3) * (Wo + 3) * 16].to(F64).view(F, Ho + 3, Wo + 3, 16)
    B = torch.cat([R[:, s:s + Ho, t:t + Wo].reshape(-1, 16) for s in range(4) for t in range(4)], dim=1)
    idx = stem_unit_pixels(F, H, W, rec.device).flatten()
    return _slab_products(dy.to(F64)[idx], B[idx], sched)


def row_ranges(sched, rows_per_unit=128):
    return [(u0 * rows_per_unit, u1 * rows_per_unit) for u0, u1 in sched.runs]


def wgrad_bound(P, Ab, sched, c_prev=None):
    """gemm_tn_ref.bound() for fp32 slabs: the accumulation of each workgroup's run, then the fold over grid slabs (+ c_prev)."""
    return slab_bound(P, Ab, row_ranges(sched), c_prev=c_prev)


# ------------------------------------------------------------------------------------------------------------------ bounds
def out_bound(y0, A, K, resid=None):
    """-> (ref, Epre, Estore) float64 [M][64]: the value before the store, its bound, and the bound of the stored bf16."""
    E = (K + 2) * U * A
    ref = y0
    if resid is not None:
        ref = y0 + resid.to(F64)
        E = E + U * (ref.abs() + E)
    return ref, E, E + half_ulp_bf16(ref.abs() + E)


def group_sums(v, groups):
    """v [M][64] -> [len(groups)][64]: sums over the rows of every group; groups long [G][n] of row indices."""
    return v[groups.flatten()].view(groups.shape[0], groups.shape[1], -1).sum(1)


def stats_ref_and_bound(ref, Epre, groups):
    """The table rows of `groups` (long [G][n] row indices, all of one length n) -> (sums, squares, bound of sums, bound of squares)."""
    n = groups.shape[1]
    mag = ref.abs() + Epre
    s1, s2 = group_sums(ref, groups), group_sums(ref * ref, groups)
    b1 = group_sums(Epre, groups) + (n + 2) * U * group_sums(mag, groups)
    b2 = group_sums(2 * ref.abs() * Epre + Epre * Epre, groups) + (n + 3) * U * group_sums(mag * mag, groups)
    return s1, s2, b1, b2


def stats_by_runs(ref, Epre, runs, unit_rows):
    """Statistics of runs of DIFFERENT lengths: runs [(u0, u1)] of units whose rows are unit_rows long [units][128].
    -> (sums, squares, bound of sums, bound of squares), each [len(runs)][64]; grouped by run length."""
    out = [torch.zeros(len(runs), ref.shape[1], dtype=F64, device=ref.device) for _ in range(4)]
    by_len = {}
    for i, (u0, u1) in enumerate(runs):
        by_len.setdefault(u1 - u0, []).append(i)
    for n, idx in by_len.items():
        groups = torch.stack([unit_rows[runs[i][0]:runs[i][1]].flatten() for i in idx])
        for o, r in zip(out, stats_ref_and_bound(ref, Epre, groups)):
            o[torch.tensor(idx, device=ref.device)] = r
    return out


def worst(got, want, bnd):
    """-> (largest err / bound, offenders, flat index of the worst element).  NaN counts as an offender."""
    err = (got.to(F64) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    bad = int((~(err <= bnd)).sum())
    flat = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")).flatten()
    k = int(flat.argmax())
    return float(flat[k]), bad, k


def describe_pixel(kind, case, sched, k):
    """Element k of a forward output [M][64] in words: frame / y / x / channel, tile or unit, workgroup, position in the run."""
    p, ch = k // 64, k % 64
    if kind == "conv":
        F, H, W = case.F, case.H, case.W
        f, y, x = p // (H * W), p % (H * W) // W, p % W
        u = p // 256
        name = "tile"
    else:
        Ho, Wo = stem_geometry(case.H, case.W)
        f, y, x = p // (Ho * Wo), p % (Ho * Wo) // Wo, p % Wo
        u = (f * (Wo // 128) + x // 128) * Ho + y
        name = "unit"
    wg, pos = sched.where(u)
    return f"pixel {p} (frame {f}, y {y}, x {x}) channel {ch}, {name} {u}, workgroup {wg}, position {pos} of its run of {sched.per}"


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    """One geometry.  conv cases: tokens (F, H, W); stem cases: IMAGES (F, H, W).  props: the properties of the launcher's schedule the
    case exists for - properties() must return exactly these values (tests/test_conv_halo_ref.py asserts it)."""
    kind: str           # 'conv' | 'wgrad' | 'stem'
    F: int
    H: int
    W: int
    why: str
    props: tuple        # ((key, value), ...)

    @property
    def name(self):
        return f"{self.kind}_{self.F}x{self.H}x{self.W}"

    def schedule(self):
        return {"conv": fwd_schedule, "wgrad": wgrad_schedule, "stem": stem_schedule}[self.kind](self.F, self.H, self.W)


def refills(sched, buffer):
    """Forward kernel: how often a frame's LAST tile (zero bottom halo row) is loaded into halo buffer `buffer` after that buffer held
    a tile with a real bottom row (the tile two places earlier in the run)."""
    n = 0
    for u0, u1 in sched.runs:
        for u in range(u0 + 2, u1):
            if (u - u0) % 2 == buffer and u % sched.upf == sched.upf - 1 and (u - 2) % sched.upf != sched.upf - 1:
                n += 1
    return n


def properties(c):
    """Everything a case may record, from its schedule alone."""
    s = c.schedule()
    runs = [r for r in s.runs if r[1] > r[0]]
    p = {"units": s.units, "upf": s.upf, "per": s.per, "grid": s.grid, "empty": len(s.runs) - len(runs), "cross": s.crossing(),
         "short_last": runs[-1][1] - runs[-1][0] < s.per}
    longest = max(b - a for a, b in s.stretches())
    if c.kind == "conv":
        p.update(refill0=refills(s, 0), refill1=refills(s, 1), second_buffer=any(b - a >= 2 for a, b in runs))
    elif c.kind == "wgrad":
        tyu = 128 // c.W
        p.update(ring=ring_slots(c.W), wraps=longest * tyu + 2 > ring_slots(c.W))      # rows y0 - 1 .. of a stretch exceed the slots
    else:
        Ho, Wo = stem_geometry(c.H, c.W)
        # a stretch of n units passes rows oy .. oy + n + 2 through slots (row & 7): it wraps when it runs past slot 7, and it overwrites
        # a slot it filled itself from n = 6 on
        p.update(Ho=Ho, Wo=Wo, strips=Wo // 128, wraps=any((a % s.upf) % 8 + (b - a) + 2 >= 8 for a, b in s.stretches()),
                 overwrites=longest >= 6)
    return p


def _c(kind, shape, why, **props):
    return Case(kind, *shape, why, tuple(sorted(props.items())))


def conv_cases():
    out = [_c("conv", s, "one tile per frame: both vertical halo rows are zero", upf=1, per=1, units=3)
           for s in ((3, 2, 128), (3, 4, 64), (3, 8, 32), (3, 16, 16))]
    out.append(_c("conv", (1, 6, 128), "first, middle and last tile of one frame", upf=3, units=3, per=1))
    out.append(_c("conv", (300, 16, 16), "per = 2; 106 workgroups return with no tile, yet every table row must be written",
                  per=2, units=300, empty=106, upf=1))
    out.append(_c("conv", (6, 86, 128), "per = 2, runs cross frames: the weights-then-halo second buffer at W = 128", per=2, units=258,
                  upf=43, second_buffer=True, cross=3))
    for s in ((103, 10, 128), (103, 20, 64), (103, 40, 32), (103, 80, 16)):
        out.append(_c("conv", s, "515 tiles, 5 per frame, per = 3: 68 runs cross a frame; a frame's last tile refills buffer 0 after a "
                      "tile with a real bottom row; the last run is short", units=515, upf=5, per=3, cross=68, refill0=34, short_last=True))
    for s in ((154, 10, 128), (154, 80, 16)):
        out.append(_c("conv", s, "per = 4: the same refill in buffer 1", units=770, upf=5, per=4, refill1=38))
    return out


def wgrad_cases():
    out = [_c("wgrad", s, "one unit per frame: every unit is a full reload", upf=1, per=1, units=5, cross=0)
           for s in ((5, 1, 128), (5, 2, 64), (5, 4, 32))]
    for s in ((86, 3, 128), (86, 6, 64), (86, 12, 32)):
        out.append(_c("wgrad", s, "258 units, per = 2: 43 runs change frame mid-run", units=258, upf=3, per=2, cross=43, grid=129))
    for s in ((147, 7, 128), (147, 14, 64), (147, 28, 32)):
        out.append(_c("wgrad", s, "1029 units, per = 5: 117 runs cross a frame, in-frame stretches of 5 units wrap the ring", units=1029,
                      upf=7, per=5, cross=117, wraps=True, grid=206, short_last=True))
    for g in (1, 15, 16, 17, 48, 49, 64, 65, 113):
        out.append(_c("wgrad", (g, 1, 128), "slab count at an edge of chw_fold_kernel's unrolled and tail loops", grid=g, per=1))
    return out


def stem_cases():
    return [_c("stem", (2, 1, 255), "Ho = 1", Ho=1, Wo=128, units=2, per=1),
            _c("stem", (2, 2, 256), "Ho = 1", Ho=1, Wo=128, units=2, per=1),
            _c("stem", (1, 5, 767), "Wo = 384: three strips", Ho=3, Wo=384, strips=3, units=9),
            _c("stem", (1, 37, 255), "odd sizes", Ho=19, Wo=128, per=1),
            _c("stem", (3, 173, 256), "Ho = 87, per = 2: one run crosses a strip", Ho=87, per=2, cross=1, units=261),
            _c("stem", (2, 259, 512), "Ho = 130, per = 3, two strips per frame", Ho=130, per=3, strips=2, units=520),
            _c("stem", (4, 257, 512), "Ho = 129, per = 5: six runs cross a strip; stretches of 5 fill all 8 ring slots and wrap", Ho=129,
               per=5, cross=6, units=1032, wraps=True, overwrites=False),
            _c("stem", (5, 513, 256), "Ho = 257, per = 6: a stretch of 6 overwrites the ring slot of its own first row", Ho=257, per=6,
               units=1285, overwrites=True)]


def cases():
    out = conv_cases() + wgrad_cases() + stem_cases()
    assert len({c.name for c in out}) == len(out)
    return out


FLAVOURS = ("signed", "nonneg")


def _flav(t, flavour):
    return t.abs() if flavour == "nonneg" else t


def conv_problem(c, flavour="signed"):
    """CPU operands of a conv3x3_c64 case: x / dy [M][64] bf16, resid [M][64] bf16, w (64, 64, 3, 3) bf16-representable fp32 (outputs of
    magnitude ~1), fwd / dgrad matrices built from it by conv_wmats()."""
    g = torch.Generator().manual_seed(1000 * c.F + 10 * c.H + c.W)
    M = c.F * c.H * c.W
    x = _flav(torch.randn(M, 64, generator=g), flavour).to(BF)
    resid = _flav(torch.randn(M, 64, generator=g), flavour).to(BF)
    w = _flav(torch.randn(64, 64, 3, 3, generator=g) / 24, flavour).to(BF)
    fwd, dg = conv_wmats(w)
    return {"x": x, "resid": resid, "fwd": fwd, "dgrad": dg, "w": w}


def wgrad_problem(c):
    g = torch.Generator().manual_seed(2000 * c.F + 10 * c.H + c.W)
    M = c.F * c.H * c.W
    return {"dy": torch.randn(M, 64, generator=g).to(BF), "x": torch.randn(M, 64, generator=g).to(BF),
            "prev": torch.randn(64, 576, generator=g)}


def stem_problem(c, flavour="signed"):
    """CPU operands of a stem case: a DENSE record buffer (64 trailing values included), a dense W [64][256], dy, c_prev."""
    g = torch.Generator().manual_seed(3000 * c.F + 10 * c.H + c.W)
    Ho, Wo = stem_geometry(c.H, c.W)
    n = c.F * (Ho + 3) * (Wo + 3) * 16 + 64
    return {"rec": _flav(torch.randn(n, generator=g), flavour).to(BF), "w": _flav(torch.randn(64, 256, generator=g) / 16, flavour).to(BF),
            "dy": torch.randn(c.F * Ho * Wo, 64, generator=g).to(BF), "prev": torch.randn(64, 256, generator=g)}
