"""stswin_gemm_tn (stswincl_amd/csrc/gemm.hip: gemm_tn_kernel<T, 4|8>, gemm_tn_ring_kernel<0..3>, gemm_tn_rows_kernel, every way the
split contraction is combined) against the float64 contract of tests/gemm_tn_ref.py - per ELEMENT, with the derived bound of that
module (nothing here is tuned on a GPU).  The cases are gemm_tn_ref.cases(): the smallest shapes at which each path can still go wrong;
tests/test_gemm_tn_ref.py shows on the CPU that at every one of them a dropped contraction row, a -1 map row read as row 0, a tap read
through its neighbour's map and a missing tap-minor permutation land outside the bound.

Every case, once overwriting a NaN-filled C and once accumulating onto a random one, asserts
  * which kernel and which combine form ran: the raw stswin_last_variant(1) word - kernel code, fp32 / bf16 slabs, fused, tap-minor, and
    the split count in bits 16 and up; the partition handed to the bound comes from that count.  A case that lands elsewhere fails;
  * |got - ref| <= bound for every element; a failure names the worst element, its tile-local position, the split whose partial comes
    closest to the error and the number of offenders; one line per case is printed with the largest err / bound;
  * nothing else was written: C is a column slice (from column 4) of a taller, wider fp32 buffer filled with a finite sentinel - the rows
    past Ni and the columns on either side are bit-identical afterwards, with a pitch that is a multiple of 4 and, where slabs are
    combined, with one that is not (the scalar store paths of tn_reduce_kernel and of the fused combine); At, Bt and both maps likewise;
  * the shared split-K workspace is NaN before every launch and the result is finite: no stale partial is read;
  * a second call gives the same bits (fp32 atomics over several splits excepted)."""
import dataclasses

import pytest
import torch

import gemm_tn_ref as T
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
F64 = torch.float64
SENT = 12345.0
COL0 = 4
DEV = "cuda"
CASES = T.cases()
BY_NAME = {c.name: c for c in CASES}
_REF = {}                                                  # case -> its operands and float64 partials: computed once, never changed


def _id(c):
    return c.name.replace(" ", "_")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _decode(w):
    k = w & 0xFFF
    return (f"{T.KERNEL_NAMES.get(k, k)}" + (" slabs_f32" if w & T.SLABS_F32 else "") + (" slabs_bf16" if w & T.SLABS_BF16 else "") +
            (" fused" if w & T.FUSED else "") + (" tapminor" if w & T.TAPMINOR else "") + f" splits={w >> 16}")


def _reference(c):
    if c not in _REF:
        p = T.problem(c)
        A, B = T.operands(p["At"], p["Bt"], Mk=c.Mk, Nj=c.Nj, at_rows=p["at_rows"], bt_rows=p["bt_rows"], bseg=c.bseg)
        P, Ab = T.partials(A, B, c.ranges())
        if c.tapminor_honoured:
            P, Ab = T.to_tapminor(P, c.bseg), T.to_tapminor(Ab, c.bseg)
        g = torch.Generator().manual_seed(c.Mk + c.Nj)
        _REF[c] = (p, P, Ab, torch.randn(c.Ni, c.Nj, generator=g))
    return _REF[c]


def _launch(c, d, Cview, overwrite):
    """One call as the case asks for it -> the raw variant word.  d: the operands on the device."""
    ws = hip._tn_workspace(torch.device(DEV, torch.cuda.current_device()))
    ws.fill_(float("nan"))                                 # stale partials must not leak into the result
    nocombine = c.form.startswith("nocombine")
    splits = c.req | c.bits | (hip.TN_NO_COMBINE if nocombine else 0)
    hip.gemm_tn(d["At"], d["Bt"], Cview, Mk=c.Mk, at_rows=d["at_rows"], bt_rows=d["bt_rows"], splits=splits, bseg=c.bseg,
                atomics=c.form == "atomics", overwrite=overwrite, tapminor=c.tapminor)
    word = hip.load().stswin_last_variant(1)
    if nocombine and word & (T.SLABS_F32 | T.SLABS_BF16):  # the partials wait in the workspace: combine them as the word says
        rc = hip.load().stswin_tn_combine(ws.data_ptr(), Cview.data_ptr(), Cview.stride(0), c.Ni, c.Nj, word >> 16, 1 if overwrite else 0,
                                          1 if word & T.SLABS_BF16 else 0, hip._stream())
        assert rc == 0, f"{c.name}: stswin_tn_combine returned {rc}"
    return word


def run_case(c, monkeypatch, record=None):
    """One case of gemm_tn_ref.cases(), checked as the module docstring says -> {(overwrite, pitch): bits of the C slice}."""
    p, P, Ab, prev = _reference(c)
    d = {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}
    pitch4 = (COL0 + c.Nj + 8 + 3) // 4 * 4
    pitches = [pitch4] + ([pitch4 + 1] if c.has_slabs else [])
    want0 = P.sum(0)
    out, line, fails = {}, [f"{c.name} [{c.expect}]"], []
    with monkeypatch.context() as mp:
        mp.delenv("STSWIN_TN_F32_SLABS", raising=False)
        mp.delenv("STSWIN_TN_FUSED", raising=False)
        if c.form in ("f32slabs", "nocombine+f32"):
            mp.setenv("STSWIN_TN_F32_SLABS", "1")
        if c.form == "unfused":
            mp.setenv("STSWIN_TN_FUSED", "0")
        for overwrite in (True, False):
            for pitch in pitches:
                tag = f"{c.name} ({'overwrite' if overwrite else 'accumulate'}, pitch {pitch})"
                Cinit = torch.full((c.Ni + 3, pitch), SENT)
                Cinit[:c.Ni, COL0:COL0 + c.Nj] = float("nan") if overwrite else prev
                runs = []
                for _ in range(2):
                    Cb = Cinit.to(DEV, copy=True)
                    word = _launch(c, d, Cb[:c.Ni, COL0:COL0 + c.Nj], overwrite)
                    runs.append((word, Cb.cpu()))
                word, Cb = runs[0]
                assert word == c.word, f"{tag}: ran {_decode(word)} (0x{word:x}), the case is {_decode(c.word)} (0x{c.word:x})"
                got = Cb[:c.Ni, COL0:COL0 + c.Nj]
                assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} elements are not finite"
                inside = torch.zeros(c.Ni + 3, pitch, dtype=torch.bool)
                inside[:c.Ni, COL0:COL0 + c.Nj] = True
                stray = (_bits(Cb) != _bits(Cinit)) & ~inside
                assert not bool(stray.any()), (f"{tag}: {int(stray.sum())} elements outside the result were written, first at "
                                               f"{tuple(int(x) for x in stray.nonzero()[0])} of a {tuple(Cb.shape)} buffer")
                cp = None if overwrite else prev
                bnd = T.bound(P, Ab, c.ranges(), c_prev=cp, slab_bf16=bool(word & T.SLABS_BF16), rows_kernel=c.rows)
                want = want0 if overwrite else prev.double() + want0
                ratio, bad, where = T.worst(got, want, bnd, P, tile=c.tile, tapminor_bseg=c.bseg if word & T.TAPMINOR else 0)
                line.append(f"{'ow' if overwrite else 'acc'}{pitch % 4} {ratio:.3f}")
                if record is not None:
                    record[c.expect] = max(record.get(c.expect, 0.0), ratio)
                if bad:
                    fails.append(f"{tag}: {bad} of {got.numel()} elements beyond their bound, worst err / bound = {ratio:.3g} at {where}")
                word2, Cb2 = runs[1]
                assert word2 == word
                if c.expect != "atomics":
                    assert torch.equal(_bits(Cb2), _bits(Cb)), f"{tag}: a second call gave other bits"
                out[(overwrite, pitch % 4)] = _bits(got).clone()
    print("[gemm_tn] " + "  ".join(line))
    assert not fails, "; ".join(fails)
    for k, v in p.items():                                 # the inputs are untouched
        assert v is None or torch.equal(_bits(d[k].cpu()), _bits(v)), f"{c.name}: {k} was written"
    return out


# ---------------------------------------------------------------------------------------------------- every case but the automatic one
@pytest.mark.parametrize("c", [c for c in CASES if c.Mk != 22528], ids=_id)
def test_case(c, monkeypatch):
    run_case(c, monkeypatch)


# ---------------------------------------------------------------------------------------------------- fused == separate pass, bit for bit
@pytest.mark.parametrize("c", [c for c in CASES if c.expect == "fused" and c.Mk != 22528], ids=_id)
def test_fused_combine_is_bitwise_the_separate_pass(c, monkeypatch):
    other = BY_NAME[c.name + " unfused"]
    assert other.expect == "bf16" and dataclasses.replace(other, name=c.name, form="") == c
    a, b = run_case(c, monkeypatch), run_case(other, monkeypatch)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{c.name} {k}: the fused combine and tn_reduce_kernel give other bits"


def test_fused_three_times_in_a_row_on_one_stream(monkeypatch):
    """Back to back, nothing in between: the arrival / ticket / departure counters of the tiles are back at zero when a launch ends."""
    monkeypatch.delenv("STSWIN_TN_F32_SLABS", raising=False)
    monkeypatch.delenv("STSWIN_TN_FUSED", raising=False)
    for name in ("ring ragged 100x264x520 rs=2", "ring bseg=128 96x256x1152 tapminor rs=2"):
        c = BY_NAME[name]
        p, P, Ab, prev = _reference(c)
        d = {k: (v.to(DEV) if v is not None else None) for k, v in p.items()}
        hip._tn_workspace(torch.device(DEV, torch.cuda.current_device())).fill_(float("nan"))
        outs = [torch.full((c.Ni, c.Nj), float("nan"), device=DEV) for _ in range(3)]
        for o in outs:
            hip.gemm_tn(d["At"], d["Bt"], o, Mk=c.Mk, at_rows=d["at_rows"], bt_rows=d["bt_rows"], splits=c.req | c.bits, bseg=c.bseg,
                        overwrite=True, tapminor=c.tapminor)
            assert hip.load().stswin_last_variant(1) == c.word
        outs = [o.cpu() for o in outs]
        assert bool(torch.isfinite(outs[0]).all())
        assert torch.equal(_bits(outs[1]), _bits(outs[0])) and torch.equal(_bits(outs[2]), _bits(outs[0])), name
        bnd = T.bound(P, Ab, c.ranges(), slab_bf16=True)
        ratio, bad, where = T.worst(outs[2], P.sum(0), bnd, P, tile=256, tapminor_bseg=c.bseg if c.tapminor else 0)
        assert bad == 0, f"{name}: third launch in a row: {bad} elements beyond their bound, worst {where}"


# ---------------------------------------------------------------------------------------------------- the launcher's own choice
def test_automatic_dispatch_22528x512x512(monkeypatch):
    """No tuning bit, no split count: the ring kernel with bf16 slabs and the fused combine, at the split count of the launcher's own
    arithmetic - tiles x splits ~ the planned compute units (stswin_set_cu_budget; 256 by default -> 44), >= 16 stages per split."""
    c = BY_NAME["automatic dispatch 22528x512x512"]
    prev_budget = hip.load().stswin_set_cu_budget(0)
    hip.load().stswin_set_cu_budget(prev_budget)
    cus = prev_budget if prev_budget > 0 else 256
    tiles, stages = 4, c.Mk // 32
    rs = T.corrected_splits(c.Mk, max(1, min(cus // tiles, stages // 16)), 32)
    assert tiles * rs >= cus * 11 // 16, "at this budget the launcher does not pick the ring kernel: the case needs another shape"
    if cus == 256:
        assert rs == 44
    if rs != c.splits:
        c = dataclasses.replace(c, splits=rs)
    if tiles * rs > torch.cuda.get_device_properties(0).multi_processor_count:          # (more workgroups than CUs: not fused)
        c = dataclasses.replace(c, form="unfused")
        monkeypatch.setenv("STSWIN_TN_FUSED", "0")
    assert (c.word & 0xFFF) == T.RING_PLAIN and c.word & T.SLABS_BF16
    run_case(c, monkeypatch)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("code,Ni,Nj,bseg,with_map,f32", [(-1005, 136, 648, 72, True, False), (-1005, 136, 648, 72, True, True),
                                                            (-1003, 132, 264, 0, False, False), (-1004, 136, 576, 64, False, False),
                                                            (-1004, 136, 576, 64, False, True)])
def test_refusals_leave_c_untouched(code, Ni, Nj, bseg, with_map, f32):
    Mk = 200
    g = torch.Generator().manual_seed(3)
    dt = torch.float32 if f32 else torch.bfloat16
    At = torch.randn(Mk, Ni, generator=g).to(dt).to(DEV)
    Bt = torch.randn(Mk + 11, bseg or Nj, generator=g).to(dt).to(DEV)
    maps = T.conv3x3_rowmap(10, 20, 2)[:Nj // bseg].contiguous().flatten().to(DEV) if with_map else None
    Cinit = torch.full((Ni + 3, Nj + 12), SENT)
    for splits in (0, 3):
        for overwrite in (True, False):
            Cb = Cinit.to(DEV, copy=True)
            with pytest.raises(hip.StswinHipError, match=f"code {code}$"):
                hip.gemm_tn(At, Bt, Cb[:Ni, COL0:COL0 + Nj], Mk=Mk, bt_rows=maps, bseg=bseg, splits=splits, overwrite=overwrite)
            assert torch.equal(_bits(Cb.cpu()), _bits(Cinit)), f"refusal {code}: C was written"


def test_case_list_covers_every_kernel_and_combine_form():
    assert {c.kernel for c in CASES} >= {hip.VAR_TN_RING_PLAIN, hip.VAR_TN_RING_ATROWS, hip.VAR_TN_RING_BTROWS, hip.VAR_TN_RING_BSEG,
                                         hip.VAR_TN_128x128, hip.VAR_TN_128x128_W4, hip.VAR_TN_ROWS, hip.VAR_TN_128x128 + hip.VAR_F32,
                                         hip.VAR_TN_128x128_W4 + hip.VAR_F32}
    assert {c.expect for c in CASES} >= {"rows", "none", "atomics", "f32", "bf16", "fused", "explicit-f32", "explicit-bf16"}
