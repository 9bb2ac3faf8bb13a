"""tests/optim_ref.py (the float64 reference of the multi-tensor optimizer kernels) checked on the CPU before any kernel is held
against it: against torch.optim in float64, against the oracle's LARS step and the reference's own three steps (golden/lars.npz);
the fp32 emulation of the kernels against the reference (the printed units are the level expected of the kernels); and the
sensitivity of the comparator: eight deliberately wrong kernels must fail it at the bounds the GPU test holds the real ones to."""
import pytest
import torch

import golden_util as gu
import optim_ref as R
from oracle.stswin_oracle import lars_sgd_step
from test_hip_optim_contract import BOUND, exceeds

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------------------ reference vs torch
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_step_equals_float64_torch_adam(wd):
    gen = torch.Generator().manual_seed(3)
    p0 = [torch.randn(37, 5, generator=gen, dtype=F64), torch.randn(1025, generator=gen, dtype=F64)]
    a = [p.clone().requires_grad_(True) for p in p0]
    opt = torch.optim.Adam(a, 1e-3, weight_decay=wd)
    p = [x.clone() for x in p0]
    m = [torch.zeros_like(x) for x in p0]
    v = [torch.zeros_like(x) for x in p0]
    for t in range(1, 21):
        c1, c2 = R.tick_adam(t, 0.9, 0.999)
        for i in range(2):
            g = torch.randn(p0[i].shape, generator=gen, dtype=F64)
            a[i].grad = g.clone()
            p[i], m[i], v[i] = R.adam_step(p[i], g, m[i], v[i], 1e-3, 0.9, 0.999, 1e-8, wd, c1, c2)
        opt.step()
    for i in range(2):
        assert float(((p[i] - a[i].detach()).abs() / a[i].detach().abs()).max()) < 1e-12
        assert float(((m[i] - opt.state[a[i]]["exp_avg"]).abs() / opt.state[a[i]]["exp_avg"].abs()).max()) < 1e-12
        assert float((v[i] / opt.state[a[i]]["exp_avg_sq"] - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("momentum,wd", [(0.9, 0.0), (0.9, 1e-4), (0.0, 1e-4)])
def test_sgd_step_equals_float64_torch_sgd(momentum, wd):
    """20 steps from no buffer: the first step (buf = g'), the later ones, weight decay, momentum 0 (no buffer in torch)"""
    gen = torch.Generator().manual_seed(4)
    p0 = torch.randn(1025, generator=gen, dtype=F64)
    a = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([a], 0.05, momentum=momentum, weight_decay=wd)
    p, buf = p0.clone(), torch.zeros_like(p0)
    for t in range(20):
        g = torch.randn(1025, generator=gen, dtype=F64)
        a.grad = g.clone()
        p, buf = R.sgd_step(p, g, buf, 0.05, momentum, wd, first=(t == 0))
        opt.step()
        assert float(((p - a.detach()).abs() / a.detach().abs()).max()) < 1e-12, t
        if momentum:
            tb = opt.state[a]["momentum_buffer"]
            assert float(((buf - tb).abs() / tb.abs()).max()) < 1e-12, t


# ------------------------------------------------------------------------------------------------------------------ oracle, golden
@pytest.mark.parametrize("adaptive", [True, False])
def test_lars_step_equals_the_oracle_in_float64(adaptive):
    gen = torch.Generator().manual_seed(5)
    shapes = [(16, 24), (16,), (8, 4, 3, 3), (8, 16)]
    p0 = [torch.randn(*s, generator=gen, dtype=F64) for s in shapes]
    p0[3].zero_()                                     # the |p| = 0 branch
    po, bo = [x.clone() for x in p0], [None] * 4
    p, buf = [x.clone() for x in p0], [torch.zeros_like(x) for x in p0]
    for t in range(4):
        gs = [torch.randn(*s, generator=gen, dtype=F64) for s in shapes]
        if t == 1:
            gs[0].zero_()                             # norm from the decay term only
        lars_sgd_step(po, gs, bo, 0.3, 0.9, 1e-3, adaptive, 0.001, 1e-8)
        for i in range(4):
            p[i], buf[i] = R.lars_step(p[i], gs[i], buf[i], 0.3, 0.9, 1e-3, 0.001, 1e-8, t == 0, adaptive)
            assert float((p[i] - po[i]).abs().max()) <= 1e-12 * float(po[i].abs().max()), (t, i)
            assert float((buf[i] - bo[i]).abs().max()) <= 1e-12 * float(bo[i].abs().max().clamp_min(1e-300)), (t, i)


def test_lars_step_reproduces_the_reference_golden():
    """three steps of the reference's LARS(SGD(add_weight_decay(...))) (tests/golden/lars.npz), at the tolerance
    tests/test_hip_optim.py holds the kernel to"""
    g = gu.load("lars.npz")
    names = [str(n) for n in g["names"]]
    lr, mom, wd = float(g["lr"]), float(g["momentum"]), float(g["wd"])
    for n in names:
        p = torch.from_numpy(g[f"p0/{n}"])
        adaptive = p.dim() != 1
        buf = torch.zeros_like(p, dtype=F64)
        for step in range(3):
            p, buf = R.lars_step(p, torch.from_numpy(g[f"g{step}/{n}"]), buf, lr, mom, wd if adaptive else 0.0, float(g["trust_coef"]),
                                 float(g["eps"]), step == 0, adaptive)
            assert torch.allclose(p.float(), torch.from_numpy(g[f"p{step + 1}/{n}"]), rtol=2e-5, atol=1e-7), (n, step)
        assert torch.allclose(buf.float(), torch.from_numpy(g[f"buf/{n}"]), rtol=2e-5, atol=1e-7), n


def test_clock_scalars():
    assert R.tick_adam(1, 0.9, 0.999)[0] == pytest.approx(0.1, rel=1e-15)
    assert R.tick_adam(1, 0.9, 0.999)[1] == pytest.approx(0.001 ** 0.5, rel=1e-13)
    assert R.tick_ema(0, 0.99, 167625) == pytest.approx(0.99, rel=1e-15) and R.tick_ema(167625, 0.99, 167625) == 1.0
    assert R.ema(torch.tensor([2.0]), torch.tensor([4.0]), 0.75).item() == 2.5


# ------------------------------------------------------------------------------------------------------------------ emulation
def _emulate_case(case, mutation=None, sizes=R.CASE_SIZES):
    """run the emulation over `sizes` tensors of the case -> {(kind, metric, label): units}"""
    kind, label, regime, opt = case
    sc = R.scalars(kind, regime, **opt)
    res = {}
    for i, n in enumerate(sizes):
        p, g, m, v = R.values(regime, n, i, lr=sc.get("lr", 1e-3))
        got = R.emulate_fp32(kind, p, g, m, v, mutation=mutation, **sc)
        for metric, u in R.compare(kind, got, p, g, m, v, **sc).items():
            res[(kind, metric, label)] = max(res.get((kind, metric, label), 0.0), u)
    return res


EMULATED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[optim ref] fp32 emulation against the float64 reference, units of u = 2^-24 (the level expected of the kernels):")
    for k, v in sorted(EMULATED.items(), key=str):
        print(f"[optim ref]   {k}: {v:.2f}   (bound of the GPU test {BOUND[k]})")


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_emulation_is_within_the_gpu_bounds_and_the_bounds_within_4x_of_it(case):
    """the kernels' model passes the GPU test's comparator; a bound is <= 2 x what was measured on the GPU, which must be <= 2 x the
    emulation's value (the two conditions of the GPU test, as far as a CPU can check them)"""
    res = _emulate_case(case)
    for k, u in res.items():
        EMULATED[k] = max(EMULATED.get(k, 0.0), u)
        print(f"[optim ref] {R.case_id(case)} {k[1]}: {u:.2f} u")
    assert not exceeds(res), (res, {k: BOUND[k] for k in res})
    if not case[3].get("first", False):       # (first = False is the case of a shared key with more roundings)
        for k, u in res.items():
            assert BOUND[k] <= 4 * max(EMULATED[k], 0.5), (k, BOUND[k], EMULATED[k])


def _emulate_list(kind, label, sc, vals, norms_of=None):
    """the emulation over a list of tensors -> {(kind, metric, label): units}; norms_of: the tensors whose norms the GPU test reads"""
    res = {}
    for i, (p, g, m, v) in enumerate(vals):
        got = R.emulate_fp32(kind, p, g, m, v, **sc)
        for metric, u in R.compare(kind, got, p, g, m, v, **sc).items():
            if metric != "norm" or norms_of is None or i in norms_of:
                res[(kind, metric, label)] = max(res.get((kind, metric, label), 0.0), u)
    return res


def _hold_emulated(res):
    for k, u in res.items():
        EMULATED[k] = max(EMULATED.get(k, 0.0), u)
    assert not exceeds(res), (res, {k: BOUND[k] for k in res})


@pytest.mark.parametrize("kind", ["adam", "sgd", "lars", "ema"])
def test_emulation_of_the_list_length_cases(kind):
    """the inputs of test_hip_optim_contract.py::test_list_lengths, every length of the kind under one key"""
    for count in R.list_counts(kind):
        regime, sc, vals = R.list_case(kind, count)
        _hold_emulated(_emulate_list(kind, "lists", sc, vals, range((count - 1) // 48 * 48, count)))
    for k in [k for k in EMULATED if k[0] == kind and k[2] == "lists"]:
        assert BOUND[k] <= 4 * max(EMULATED[k], 0.5), (k, BOUND[k], EMULATED[k])


def test_emulation_of_the_300_chunk_case():
    sc, vals = R.big_case()
    res = _emulate_list("lars", "big", sc, vals)
    _hold_emulated(res)
    for k in res:
        assert BOUND[k] <= 4 * max(EMULATED[k], 0.5), (k, BOUND[k], EMULATED[k])


# ------------------------------------------------------------------------------------------------------------------ sensitivity
# (mutation, the cases under which it must fail the comparator at the GPU test's bounds)
def _case(kind, label, first=None):
    return next(c for c in R.cases() if c[0] == kind and c[1] == label and (first is None or c[3].get("first") == first))


SENSITIVITY = [
    ("b2", _case("adam", "unit")),
    ("b2", _case("adam", "warm")),
    ("eps_before_c2", _case("adam", "tiny_g")),
    ("no_decay", _case("adam", "warm")),
    ("no_decay", _case("adam", "zero_g")),
    ("no_decay", _case("sgd", "unit", False)),
    ("no_decay", _case("lars", "unit", False)),
    ("no_decay", _case("lars", "zero_g", False)),
    ("first_ignored", _case("sgd", "warm", True)),
    ("first_ignored", _case("lars", "warm", True)),
    ("norm_without_decay", _case("lars", "zero_g", False)),
    ("norm_without_decay", _case("lars", "unit", False)),
    ("ratio_at_zero_p", _case("lars", "zero_p", False)),
    ("tail_unwritten", _case("adam", "unit")),
    ("tail_unwritten", _case("sgd", "unit", False)),
    ("tail_unwritten", _case("ema", "unit")),
    ("ema_swapped", _case("ema", "unit")),
]


@pytest.mark.parametrize("mutation,case", SENSITIVITY, ids=[f"{m}-{R.case_id(c)}" for m, c in SENSITIVITY])
def test_a_wrong_kernel_fails_the_comparator(mutation, case):
    res = _emulate_case(case, mutation)
    bad = exceeds(res)
    print(f"[optim ref] mutation {mutation} under {R.case_id(case)}: " + " ".join(f"{k[1]}={u:.3g}" for k, u in res.items()),
          "-> over the bound:", [k[1] for k in bad])
    assert bad, (mutation, res)


def test_every_mutation_is_covered():
    assert {m for m, _ in SENSITIVITY} == set(R.MUTATIONS)


def test_the_first_step_case_needs_a_stale_buffer():
    """from a zero buffer, ignoring `first` changes nothing (momentum x 0 + g'): why the first-step cases preload the buffer"""
    c = _case("sgd", "unit", True)
    assert not exceeds(_emulate_case(c, "first_ignored"))


# ------------------------------------------------------------------------------------------------------------------ trajectories
def test_fp32_torch_drift_of_the_trajectories():
    """the bound of the GPU trajectory tests: 2 x the drift of fp32 torch (CPU) from the float64 run on the same gradients"""
    *_, d_adam = R.adam_traj_reference()
    *_, d_lars = R.lars_traj_reference()
    print(f"[optim ref] trajectory drift of fp32 torch against float64 (error over distance moved): Adam {d_adam:.3e}  LARS {d_lars:.3e}")
    assert 0 < d_adam < 1e-3 and 0 < d_lars < 1e-3
