"""The multi-tensor optimizer kernels (stswincl_amd/csrc/optim.hip: multi_tensor_kernel in its Adam, SGD-momentum, LARS and EMA
modes, mt_norms_kernel, mt_norms_fold_kernel, optim_tick_kernel) against the float64 reference of tests/optim_ref.py, called through
hip.multi_tensor, hip.multi_tensor_lars and hip.optim_tick, plus FusedAdam, LARS(FusedSGD) and ema_update.

Every comparison is ONE step from the kernel's own pre-step state: the reference gets the fp32 p, g, m, v the kernel read.  Every
element of p, m, v / the buffer and every norm is compared, in the metrics of optim_ref (units of u = 2^-24 of the rounded terms).
Tensors are views into one flat buffer per role with a run of >= 16 sentinel floats between them, which must stay bit-unchanged.

Sizes: optim_ref.SIZES (across the 4-element vector, the 1024-element sweep, the 8192-element chunk) with a zero-element tensor in
mid-list; 300 chunks + 5 for LARS (the fold kernel's strided loop).  List lengths 1, 47, 48, 49, 97 (96 for LARS: a full second
launch whose norms stay readable).  Alignment: element offsets 1, 2, 3 on each role and on all (the scalar path) equal the aligned
run bit for bit.  Regimes (optim_ref.values): unit; small_p (|p| ~ 1e-4 lr: the update dominates p); tiny_g (|g| ~ 1e-8: sqrt(v) ~
eps); warm (non-zero state, Adam corrections of t = 1000 from optim_tick); zero_g; zero_p; momentum 0; first step / later;
non-adaptive LARS without a norms tensor.

Bounds (BOUND): at most 2 x the value measured on MI355X, which is within 2 x the value of the fp32 emulation of the kernels
(optim_ref.emulate_fp32; tests/test_optim_ref.py runs it on the same inputs, prints it and checks both factors against this table).
Measured on MI355X (beside each entry of BOUND, with the emulation's value): 1 - 5 u for m, v, upd and the norms (300 chunks: 1.8 u),
equal to the emulation to the printed digits in every key but two - the kernels compute the emulation's bits, a correctly rounded
sqrt and division included.  ("ema", "upd", "unit") also holds the ema_update case, which the emulation does not run.  ("lars", "m",
"lists") is 4.48 u against 4.03 u over 338 tensors: within the factor 2 (as much as one ulp in a tensor's trust ratio moves; which
operation of the ratio differs from the emulation has not been traced).  Larger values are
cancellation in the inputs, the same in the emulation: ("sgd", "m", "unit" | "warm" | "mom0") 24.9 u is one element of the first-step
cases whose g' = g + wd p cancels to 4 % of wd p while the scale of `m` is |g'| alone; upd of "warm" / "lists" / "nonadaptive"
(5 - 10 u) are elements with |p| << 1 whose momentum x buf0 + g' cancels.  Exact cases (0 u: "zero_p" under lr = 0.5) have bound 0.
Trajectories: FusedAdam 6.756e-05, LARS(FusedSGD) 6.295e-06 of the distance moved - the figures of fp32 torch on the CPU, digit for
digit.
"""
import time

import pytest
import torch

import optim_ref as R
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SENT, SENTINEL = 16, -7.0e22

# (kind, metric, label) -> units of u.  Measured on MI355X | fp32 emulation on the CPU are listed beside each entry.
BOUND = {
    ('adam', 'm', 'lists'): 4.8,            # 2.53 | 2.53
    ('adam', 'm', 'small_p'): 3.0,          # 1.63 | 1.63
    ('adam', 'm', 'tiny_g'): 4.6,           # 2.45 | 2.45
    ('adam', 'm', 'unit'): 1.8,             # 0.95 | 0.95
    ('adam', 'm', 'warm'): 4.5,             # 2.38 | 2.38
    ('adam', 'm', 'zero_g'): 3.6,           # 1.92 | 1.92
    ('adam', 'm', 'zero_p'): 1.8,           # 0.95 | 0.95
    ('adam', 'upd', 'lists'): 14.3,         # 7.54 | 7.54
    ('adam', 'upd', 'small_p'): 5.6,        # 2.97 | 2.97
    ('adam', 'upd', 'tiny_g'): 4.6,         # 2.47 | 2.47
    ('adam', 'upd', 'unit'): 5.0,           # 2.64 | 2.64
    ('adam', 'upd', 'warm'): 3.5,           # 1.89 | 1.89
    ('adam', 'upd', 'zero_g'): 7.2,         # 3.80 | 3.80
    ('adam', 'upd', 'zero_p'): 4.7,         # 2.51 | 2.51
    ('adam', 'v', 'lists'): 8.3,            # 4.38 | 4.38
    ('adam', 'v', 'small_p'): 6.2,          # 3.28 | 3.28
    ('adam', 'v', 'tiny_g'): 9.8,           # 5.18 | 5.18
    ('adam', 'v', 'unit'): 3.6,             # 1.92 | 1.92
    ('adam', 'v', 'warm'): 6.8,             # 3.59 | 3.59
    ('adam', 'v', 'zero_g'): 3.7,           # 1.96 | 1.96
    ('adam', 'v', 'zero_p'): 3.6,           # 1.92 | 1.92
    ('ema', 'upd', 'lists'): 3.7,           # 1.97 | 1.97
    ('ema', 'upd', 'unit'): 3.7,            # 1.97 | 1.91
    ('lars', 'm', 'big'): 5.5,              # 2.94 | 2.94
    ('lars', 'm', 'lists'): 8.5,            # 4.48 | 4.03
    ('lars', 'm', 'mom0'): 7.6,             # 4.04 | 4.04
    ('lars', 'm', 'nonadaptive'): 3.6,      # 1.90 | 1.90
    ('lars', 'm', 'small_p'): 4.8,          # 2.57 | 2.57
    ('lars', 'm', 'unit'): 7.6,             # 4.04 | 4.04
    ('lars', 'm', 'warm'): 7.6,             # 4.04 | 4.04
    ('lars', 'm', 'zero_g'): 6.3,           # 3.32 | 3.32
    ('lars', 'm', 'zero_p'): 0.0,           # 0.00 | 0.00
    ('lars', 'norm', 'big'): 3.3,           # 1.76 | 1.76
    ('lars', 'norm', 'lists'): 4.6,         # 2.46 | 2.46
    ('lars', 'norm', 'mom0'): 2.6,          # 1.38 | 1.38
    ('lars', 'norm', 'small_p'): 2.5,       # 1.33 | 1.33
    ('lars', 'norm', 'unit'): 2.6,          # 1.38 | 1.38
    ('lars', 'norm', 'warm'): 2.6,          # 1.38 | 1.38
    ('lars', 'norm', 'zero_g'): 3.4,        # 1.84 | 1.84
    ('lars', 'norm', 'zero_p'): 2.5,        # 1.33 | 1.33
    ('lars', 'upd', 'big'): 4.2,            # 2.24 | 2.24
    ('lars', 'upd', 'lists'): 9.7,          # 5.12 | 5.12
    ('lars', 'upd', 'mom0'): 1.9,           # 1.04 | 1.04
    ('lars', 'upd', 'nonadaptive'): 19.7,   # 10.38 | 10.38
    ('lars', 'upd', 'small_p'): 1.8,        # 0.99 | 0.99
    ('lars', 'upd', 'unit'): 1.9,           # 1.04 | 1.04
    ('lars', 'upd', 'warm'): 3.0,           # 1.62 | 1.62
    ('lars', 'upd', 'zero_g'): 3.1,         # 1.64 | 1.64
    ('lars', 'upd', 'zero_p'): 0.0,         # 0.00 | 0.00
    ('sgd', 'm', 'lists'): 3.7,             # 1.96 | 1.96
    ('sgd', 'm', 'mom0'): 47.2,             # 24.89 | 24.89
    ('sgd', 'm', 'small_p'): 1.7,           # 0.92 | 0.92
    ('sgd', 'm', 'unit'): 47.2,             # 24.89 | 24.89
    ('sgd', 'm', 'warm'): 47.2,             # 24.89 | 24.89
    ('sgd', 'm', 'zero_g'): 3.6,            # 1.93 | 1.93
    ('sgd', 'm', 'zero_p'): 0.0,            # 0.00 | 0.00
    ('sgd', 'upd', 'lists'): 8.9,           # 4.71 | 4.71
    ('sgd', 'upd', 'mom0'): 2.5,            # 1.35 | 1.35
    ('sgd', 'upd', 'small_p'): 1.9,         # 1.02 | 1.02
    ('sgd', 'upd', 'unit'): 2.5,            # 1.35 | 1.35
    ('sgd', 'upd', 'warm'): 16.7,           # 8.80 | 8.80
    ('sgd', 'upd', 'zero_g'): 2.4,          # 1.28 | 1.28
    ('sgd', 'upd', 'zero_p'): 0.9,          # 0.49 | 0.49
}
MEASURED = {}


def exceeds(res):
    """the keys of res = {(kind, metric, label): units} that are over their bound"""
    return [k for k, u in res.items() if not u <= BOUND[k]]


def _hold(res):
    for k, u in res.items():
        MEASURED[k] = max(MEASURED.get(k, 0.0), u)
    print("[optim] " + "  ".join(f"{k}: {u:.2f}" for k, u in res.items()))
    bad = exceeds(res)
    assert not bad, {k: (res[k], BOUND[k]) for k in bad}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[optim contract] wall time {time.perf_counter() - t0:.1f} s; measured maxima (units of u = 2^-24):")
    for k, v in sorted(MEASURED.items(), key=str):
        print(f"[optim]   {k}: {v:.2f}")


# ------------------------------------------------------------------------------------------------------------------ layouts
ROLES = {"adam": "pgmv", "sgd": "pgm", "lars": "pgm", "ema": "pg"}


class Layout:
    """tensors of `sizes` elements as views into one flat fp32 buffer per role, each view `offs[role]` elements past a 16-byte
    boundary, >= 16 sentinel floats before, between and after the views"""

    def __init__(self, kind, vals, offs=None):
        self.kind, self.sizes = kind, [t[0].numel() for t in vals]
        offs = offs or {}
        pos, starts = SENT, []
        for n in self.sizes:
            starts.append(pos)
            pos = (pos + 3 + n + 3) // 4 * 4 + SENT
        self.flat, self.views, self.inside = {}, {}, {}
        for r, role in enumerate("pgmv"):
            if role not in ROLES[kind]:
                continue
            off = offs.get(role, 0)
            flat = torch.full((pos,), SENTINEL, dtype=F32)
            inside = torch.zeros(pos, dtype=torch.bool)
            for s, n, t in zip(starts, self.sizes, vals):
                flat[s + off:s + off + n] = t[r]
                inside[s + off:s + off + n] = True
            self.flat[role] = flat.cuda()
            assert self.flat[role].data_ptr() % 16 == 0
            self.inside[role] = inside.cuda()
            self.views[role] = [self.flat[role][s + off:s + off + n] for s, n in zip(starts, self.sizes)]
        self.before = {role: [t.clone() for t in vs] for role, vs in self.views.items()}      # what the kernel reads

    def lists(self):
        return [self.views.get(role) for role in "pgmv"]

    def check_untouched(self):
        for role, flat in self.flat.items():
            assert bool((flat[~self.inside[role]] == SENTINEL).all()), f"a sentinel of role {role} changed"
        assert all(torch.equal(a, b) for a, b in zip(self.views["g"], self.before["g"])), "the gradient / query was written"

    def bits(self):
        """the written roles, each as one tensor (for bitwise comparisons between runs)"""
        return {role: torch.cat(self.views[role]) for role in ROLES[self.kind] if role != "g"}


def _vals(kind, regime, sizes, sc, seed0=0):
    return [R.values(regime, n, seed0 + i, lr=sc.get("lr", 1e-3)) for i, n in enumerate(sizes)]


def _norms_buffer(sizes):
    """caller-owned LARS scratch for the largest 48-tensor launch over `sizes`, sentinel-filled, with 16 floats more"""
    need = max(2 * len(sizes[lo:lo + 48]) + 2 * sum((n + R.CHUNK - 1) // R.CHUNK for n in sizes[lo:lo + 48]) for lo in range(0, len(sizes), 48))
    return torch.full((need + SENT,), SENTINEL, dtype=F32, device="cuda"), need


def _hyper(sc):
    return torch.tensor([sc.get("lr", 0.0), sc.get("c1", 0.0), sc.get("c2", 0.0), sc.get("b1", 0.0)], dtype=F32).cuda()


def _launch(kind, L, sc, *, dev=False, norms=None):
    """one launch over the layout; dev: the step-dependent scalars from a device `hyper`, their arguments left at values that
    would be wrong"""
    ps, gs, ms, vs = L.lists()
    hyper = _hyper(sc) if dev else None
    if kind == "adam":
        kw = dict(b1=sc["b1"], b2=sc["b2"], eps=sc["eps"], wd=sc["wd"])
        kw.update(dict(hyper=hyper) if dev else dict(lr=sc["lr"], c1=sc["c1"], c2=sc["c2"]))
        hip.multi_tensor(0, ps, gs, ms, vs, **kw)
    elif kind == "sgd":
        kw = dict(b1=sc["b1"], wd=sc["wd"], c1=1.0 if sc["first"] else 0.0)
        kw.update(dict(hyper=hyper) if dev else dict(lr=sc["lr"]))
        hip.multi_tensor(1, ps, gs, ms, None, **kw)
    elif kind == "ema":
        hip.multi_tensor(2, ps, gs, **(dict(hyper=hyper, b1=0.5) if dev else dict(b1=sc["b1"])))
    else:
        hip.multi_tensor_lars(ps, gs, ms, norms, lr=-1.0 if dev else sc["lr"], momentum=sc["b1"], wd=sc["wd"], trust_coef=sc["trust"],
                              eps=sc["eps"], first=sc["first"], adaptive=sc["adaptive"], hyper=hyper)


def _compare(kind, label, L, sc, norms=None, norms_of=None):
    """every tensor of the layout against the float64 step from what the kernel read -> {(kind, metric, label): units};
    norms_of: the tensor indices norms[0], norms[1], .. belong to (default: all, in order)"""
    res = {}
    b = L.before
    nidx = {t: j for j, t in enumerate(norms_of if norms_of is not None else range(len(L.sizes)))}
    for i in range(len(L.sizes)):
        got = {"p": L.views["p"][i]}
        if "m" in L.views:
            got["m"] = L.views["m"][i]
        if "v" in L.views:
            got["v"] = L.views["v"][i]
        have_norms = norms is not None and i in nidx
        if have_norms:
            got["norms"] = norms[2 * nidx[i]:2 * nidx[i] + 2]
        elif kind == "lars" and sc["adaptive"]:
            got["norms"] = torch.tensor(R.lars_norms(b["p"][i], b["g"][i], sc["wd"]), dtype=F64)     # (not readable: not compared)
        one = R.compare(kind, got, b["p"][i], b["g"][i], b["m"][i] if "m" in b else None, b["v"][i] if "v" in b else None, **sc)
        for metric, u in one.items():
            if metric == "norm" and not have_norms:
                continue
            res[(kind, metric, label)] = max(res.get((kind, metric, label), 0.0), u)
    return res


# ------------------------------------------------------------------------------------------------------------------ the regimes
def _device_adam_corrections(t):
    """c1, c2 of step t as the device makes them: the counter seeded to t - 1, one optim_tick"""
    counter = torch.full((1,), t - 1, dtype=torch.int32, device="cuda")
    hyper = torch.zeros(4, dtype=F32, device="cuda")
    hip.optim_tick(0, counter, hyper, 0.9, 0.999)
    assert int(counter) == t
    return float(hyper[1]), float(hyper[2])


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_one_step_against_float64(case):
    """every size of SIZES and an empty tensor in mid-list, 16-byte aligned, by-value scalars (Adam "warm": the corrections of
    t = 1000 made by optim_tick, read through `hyper`)"""
    kind, label, regime, opt = case
    sc = R.scalars(kind, regime, **opt)
    dev = kind == "adam" and regime == "warm"
    if dev:
        c1, c2 = _device_adam_corrections(R.ADAM_T["warm"])
        assert abs(c1 / sc["c1"] - 1) <= 2 ** -23 and abs(c2 / sc["c2"] - 1) <= 2 ** -23
        sc.update(c1=c1, c2=c2)
    sizes = R.CASE_SIZES
    L = Layout(kind, _vals(kind, regime, sizes, sc))
    norms = None
    if kind == "lars" and sc["adaptive"]:
        norms, need = _norms_buffer(sizes)
    _launch(kind, L, sc, dev=dev, norms=norms)
    L.check_untouched()
    if norms is not None:
        assert bool((norms[need:] == SENTINEL).all())
        z = sizes.index(0)
        assert norms[2 * z:2 * z + 2].tolist() == [0.0, 0.0]           # the empty tensor: norms 0 (hence ratio 1)
    _hold(_compare(kind, label, L, sc, norms))


# ------------------------------------------------------------------------------------------------------------------ list lengths
@pytest.mark.parametrize("kind,count", [(k, c) for k in ("adam", "sgd", "lars", "ema") for c in R.list_counts(k)])
def test_list_lengths(kind, count):
    """one, two and three launches of up to 48 tensors; LARS: the norms of the last launch are read back from the caller's scratch
    (at 96 a full second launch, at 49 and 97 one tensor), every other norm shows in the update it scales"""
    regime, sc, vals = R.list_case(kind, count)
    sizes = R.list_sizes(count)
    L = Layout(kind, vals)
    norms, norms_of = None, None
    if kind == "lars":
        norms, need = _norms_buffer(sizes)
        norms_of = list(range((count - 1) // 48 * 48, count))
    _launch(kind, L, sc, norms=norms)
    L.check_untouched()
    _hold(_compare(kind, "lists", L, sc, norms, norms_of))


def test_lars_norms_of_a_300_chunk_tensor():
    """per-block partials, the fold's block offset for tensors after the big one and its strided loop (> 256 partials)"""
    sc, vals = R.big_case()
    L = Layout("lars", vals)
    norms, need = _norms_buffer(R.LARS_BIG_LIST)
    _launch("lars", L, sc, norms=norms)
    L.check_untouched()
    assert bool((norms[need:] == SENTINEL).all())
    res = _compare("lars", "big", L, sc, norms)
    _hold(res)


# ------------------------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("kind", ["adam", "sgd", "lars", "ema"])
def test_unaligned_views_give_the_aligned_bits(kind):
    """element offsets 1, 2, 3 on one role at a time and on all: the scalar path of multi_tensor_kernel / mt_norms_kernel evaluates
    the expression of the vector path"""
    regime = "unit" if kind == "ema" else "warm"
    sc = R.scalars(kind, regime, first=False) if kind in ("sgd", "lars") else R.scalars(kind, regime)
    sizes = R.CASE_SIZES
    vals = _vals(kind, regime, sizes, sc, seed0=5)

    def run(offs):
        L = Layout(kind, vals, offs)
        norms = _norms_buffer(sizes)[0] if kind == "lars" else None
        _launch(kind, L, sc, norms=norms)
        L.check_untouched()
        out = L.bits()
        if norms is not None:
            out["norms"] = norms[:2 * len(sizes)].clone()
        return out

    want = run({})
    for roles in list(ROLES[kind]) + [ROLES[kind]]:
        for off in (1, 2, 3):
            got = run({r: off for r in roles})
            for key in want:
                assert torch.equal(got[key], want[key]), (roles, off, key)


@pytest.mark.parametrize("kind", ["adam", "sgd", "ema"])
def test_chunking_invariance(kind):
    """the same values as one tensor or split across four: the same bits"""
    regime = "unit" if kind == "ema" else "warm"
    sc = R.scalars(kind, regime, first=False) if kind == "sgd" else R.scalars(kind, regime)
    parts = [8193, 1, 4099, 12288]
    whole = R.values(regime, sum(parts), 9, lr=sc.get("lr", 1e-3))
    split, lo = [], 0
    for n in parts:
        split.append(tuple(t[lo:lo + n] for t in whole))
        lo += n
    outs = []
    for vals in ([whole], split):
        L = Layout(kind, vals)
        _launch(kind, L, sc)
        L.check_untouched()
        outs.append(L.bits())
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), key


# ------------------------------------------------------------------------------------------------------------------ call forms
@pytest.mark.parametrize("kind", ["adam", "sgd", "lars", "ema"])
def test_scalars_by_value_and_from_device_memory_give_the_same_bits(kind):
    """stswin_multi_tensor / stswin_multi_tensor_lars against their _dev twins with the same fp32 values in `hyper`"""
    regime = "unit" if kind == "ema" else "warm"
    sizes = R.CASE_SIZES
    for first in ((True, False) if kind in ("sgd", "lars") else (None,)):
        sc = R.scalars(kind, regime, first=first) if first is not None else R.scalars(kind, regime)
        vals = _vals(kind, regime, sizes, sc, seed0=3)
        outs = []
        for dev in (False, True):
            L = Layout(kind, vals)
            norms = _norms_buffer(sizes)[0] if kind == "lars" else None
            _launch(kind, L, sc, dev=dev, norms=norms)
            L.check_untouched()
            outs.append(L.bits())
            if norms is not None:
                outs[-1]["norms"] = norms[:2 * len(sizes)].clone()
        for key in outs[0]:
            assert torch.equal(outs[0][key], outs[1][key]), (first, key)
        if first:                                        # the first step may not depend on the stale buffer
            L2 = Layout(kind, [(p, g, m + 1.0, v) for p, g, m, v in vals])
            _launch(kind, L2, sc, norms=_norms_buffer(sizes)[0] if kind == "lars" else None)
            assert torch.equal(L2.bits()["p"], outs[0]["p"]) and torch.equal(L2.bits()["m"], outs[0]["m"])


@pytest.mark.parametrize("dev", [False, True], ids=["argument", "hyper3"])
def test_ema_momentum_one_keeps_the_key_and_zero_copies_the_query(dev):
    sizes = R.CASE_SIZES
    vals = _vals("ema", "unit", sizes, {}, seed0=8)
    for mom in (1.0, 0.0):
        L = Layout("ema", vals)
        _launch("ema", L, dict(b1=mom), dev=dev)
        L.check_untouched()
        want = L.before["p"] if mom == 1.0 else L.before["g"]
        assert torch.equal(torch.cat(L.views["p"]).view(torch.int32), torch.cat(want).view(torch.int32)), mom


def test_ema_update_one_step():
    from stswincl_amd.optim import ema_update
    sc = R.scalars("ema", "unit")
    sizes = R.list_sizes(49)
    L = Layout("ema", _vals("ema", "unit", sizes, sc, seed0=21))
    ema_update([torch.nn.Parameter(k, requires_grad=False) for k in L.views["p"]], L.views["g"], sc["b1"])
    L.check_untouched()
    _hold(_compare("ema", "unit", L, sc))


# ------------------------------------------------------------------------------------------------------------------ optim_tick
def _is_fp32_of(x, want):
    """x (an fp32 value) is the float64 `want` rounded to fp32, or a neighbour of it"""
    w = torch.tensor(want, dtype=F64).float()
    nb = [float(torch.nextafter(w, torch.tensor(s, dtype=F32))) for s in (-float("inf"), float("inf"))]
    return x == float(w) or x in nb


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 10 ** 5, 10 ** 6])
def test_optim_tick_adam(t):
    counter = torch.full((1,), t - 1, dtype=torch.int32, device="cuda")
    hyper = torch.tensor([0.125, -1.0, -1.0, 0.75], dtype=F32, device="cuda")
    hip.optim_tick(0, counter, hyper, 0.9, 0.999)
    c1, c2 = R.tick_adam(t, 0.9, 0.999)
    h = hyper.tolist()
    assert int(counter) == t
    assert _is_fp32_of(h[1], c1) and _is_fp32_of(h[2], c2), (h, c1, c2)
    assert h[0] == 0.125 and h[3] == 0.75


@pytest.mark.parametrize("k", [0, 167625 // 2, 167625 - 1, 167625])
def test_optim_tick_ema(k):
    K = 167625
    counter = torch.full((1,), k, dtype=torch.int32, device="cuda")
    hyper = torch.tensor([0.125, 0.25, 0.5, -1.0], dtype=F32, device="cuda")
    hip.optim_tick(1, counter, hyper, 0.99, float(K))
    h = hyper.tolist()
    assert int(counter) == k + 1
    assert _is_fp32_of(h[3], R.tick_ema(k, 0.99, K)), (h, R.tick_ema(k, 0.99, K))
    if k == K:
        assert h[3] == 1.0
    assert h[:3] == [0.125, 0.25, 0.5]


# ------------------------------------------------------------------------------------------------------------------ trajectories
def test_fused_adam_trajectory_against_float64():
    """50 steps with weight decay, one parameter sitting out steps 10-19: error over distance moved within 2 x that of fp32
    torch.optim.Adam on the CPU from the same gradients"""
    from stswincl_amd.optim import FusedAdam
    p0, grads, p64, drift = R.adam_traj_reference()
    c = R.ADAM_TRAJ
    got = R.run_optimizer(lambda ps: FusedAdam(ps, c["lr"], weight_decay=c["wd"]), p0, grads, F32, "cuda")
    err = R.trajectory_error(got, p64, p0)
    print(f"[optim] FusedAdam trajectory: {err:.3e} (fp32 torch on the CPU: {drift:.3e})")
    assert err <= 2 * drift


def test_fused_lars_trajectory_against_float64():
    """LARS(FusedSGD(add_weight_decay(...))) for 20 steps on a module with a 25 600-element matrix (4 chunks) and 1-D parameters"""
    from stswincl_amd.contrast.lars import LARS, add_weight_decay
    from stswincl_amd.optim import FusedSGD
    names, p0, grads, p64, drift = R.lars_traj_reference()
    c = R.LARS_TRAJ
    net = R.lars_traj_module().cuda()
    params = dict(net.named_parameters())
    assert list(params) == names and all(torch.equal(params[n].detach().cpu(), p) for n, p in zip(names, p0))
    opt = LARS(FusedSGD(add_weight_decay(net, c["wd"]), lr=c["lr"], momentum=c["momentum"]), eps=c["eps"], trust_coef=c["trust"])
    for gs in grads:
        for n, g in zip(names, gs):
            params[n].grad = g.cuda()
        opt.step()
    err = R.trajectory_error([params[n] for n in names], p64, p0)
    print(f"[optim] LARS(FusedSGD) trajectory: {err:.3e} (fp32 torch on the CPU: {drift:.3e})")
    assert err <= 2 * drift


# ------------------------------------------------------------------------------------------------------------------ arguments
def _bad_tensor(n, what, role):
    """a tensor that does not match an n-element fp32 GPU parameter (as the parameter: its n-element companions), chosen so that a
    launch from it would stay in range all the same: n fp32 elements of it can be read and written, by the GPU too"""
    if what == "float64":
        return torch.zeros(n, dtype=F64, device="cuda")
    if what == "strided":
        return torch.zeros(2 * n, device="cuda")[::2]
    if what == "size":                     # a longer state for the parameter, a shorter parameter for its states
        return torch.zeros(n - 4 if role == "p" else n + 4, device="cuda")
    return torch.zeros(n).pin_memory()     # "host"


@pytest.mark.parametrize("what", ["float64", "strided", "size", "host"])
@pytest.mark.parametrize("role", ["p", "g", "m", "v"])
def test_multi_tensor_refuses_lists_that_do_not_match_the_parameters(role, what):
    n = 1025
    good = lambda: [torch.ones(8, device="cuda"), torch.ones(n, device="cuda")]  # noqa: E731
    lists = {r: good() for r in "pgmv"}
    lists[role][1] = _bad_tensor(n, what, role)
    before = [t.clone() for t in lists["p"]]
    with pytest.raises(hip.StswinHipError):
        hip.multi_tensor(0, lists["p"], lists["g"], lists["m"], lists["v"], lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, c1=0.1, c2=0.03)
    if role != "v":
        with pytest.raises(hip.StswinHipError):
            hip.multi_tensor_lars(lists["p"], lists["g"], lists["m"], None, lr=0.1, momentum=0.9, wd=0.0, trust_coef=1e-3, eps=1e-8,
                                  first=True, adaptive=True)
    if role != "p":
        assert all(torch.equal(a, b) for a, b in zip(lists["p"], before))          # raised before any launch


def test_multi_tensor_refuses_lists_of_another_length():
    ps = [torch.ones(8, device="cuda"), torch.ones(9, device="cuda")]
    with pytest.raises(hip.StswinHipError):
        hip.multi_tensor(2, ps, ps[:1], b1=0.5)
    with pytest.raises(hip.StswinHipError):
        hip.multi_tensor_lars(ps, [torch.ones_like(p) for p in ps], [torch.zeros(8, device="cuda")], None, lr=0.1, momentum=0.9, wd=0.0,
                              trust_coef=1e-3, eps=1e-8, first=True, adaptive=False)
