"""Float64 reference of the multi-tensor optimizer kernels (stswincl_amd/csrc/optim.hip): torch.optim.Adam (no amsgrad, L2 decay
joining the gradient), torch.optim.SGD with momentum (dampening 0, nesterov off), the same under LARS (contrast/lars.py around SGD),
the key-encoder EMA, and the two scalar clocks of stswin_optim_tick.

The one-step functions take the fp32 tensors a kernel reads and the scalars it receives (already rounded to fp32 where the C ABI
takes `float`: f32()), evaluate everything in float64 on the tensors' device and return float64 tensors.  emulate_fp32 evaluates the
same formulas in torch fp32 in the kernel's operation order - a model of the kernel's arithmetic (IEEE + - * / sqrt, no contraction),
whose distance from the reference is the level the kernel's is expected at.  compare() is the comparator of the CPU and GPU tests.

Error metrics, in units of u = 2^-24 times the magnitudes of the terms that were rounded (cancellation does not inflate them):
  m     |m1 - ref| / (u (|b1 m0| + |(1 - b1) g'|))      Adam exp_avg;  SGD / LARS buffer: / (u (|momentum buf0| + |g'|))
  v     |v1 / ref - 1| / u                              Adam exp_avg_sq
  upd   |(p0 - p1) - upd_ref| / (u (|upd_ref| + |p1_ref|))     the applied update (EMA: the new key, / (u (|m key| + |(1 - m) query|)))
  norm  |norm / ref - 1| / u                            LARS sum p^2, sum (g + wd p)^2
Where the scale of a metric is 0 the kernel's value must equal the reference exactly (anything else counts as infinite).
"""
import math

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
CHUNK = 8192                    # elements per block of the kernels
# the smallest set that crosses the 4-element vector, the 1024-element sweep of a block and the 8192-element chunk
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 16391, 3 * 8192]
CASE_SIZES = SIZES[:6] + [0] + SIZES[6:]       # ... with an empty tensor in mid-list: the list of every regime's launch
LARS_BIG = 300 * 8192 + 5       # more than 256 chunks: the fold kernel's strided loop
REGIMES = ["unit", "small_p", "tiny_g", "warm", "zero_g", "zero_p"]


def f32(x: float) -> float:
    """x rounded to fp32, as a Python float (what a `float` parameter of the C ABI receives)"""
    return float(torch.tensor(float(x), dtype=F32))


# ------------------------------------------------------------------------------------------------------------------ one step, float64
def adam_step(p, g, m, v, lr, b1, b2, eps, wd, c1, c2):
    """torch.optim.Adam: c1 = 1 - b1^t, c2 = sqrt(1 - b2^t) -> (p1, m1, v1)"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gr = g + wd * p
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    denom = v1.sqrt() / c2 + eps
    return p - (lr / c1) * (m1 / denom), m1, v1


def sgd_step(p, g, buf, lr, momentum, wd, first, ratio=1.0):
    """torch.optim.SGD (the kernel keeps a buffer at momentum 0, too: buf = g') -> (p1, buf1)"""
    p, g, buf = p.double(), g.double(), buf.double()
    gr = (g + wd * p) * ratio
    buf1 = gr if first else momentum * buf + gr
    return p - lr * (buf1 if momentum != 0 else gr), buf1


def lars_norms(p, g, wd):
    """-> (sum p^2, sum (g + wd p)^2) as Python floats"""
    p, g = p.double(), g.double()
    gr = g + wd * p
    return float((p * p).sum()), float((gr * gr).sum())


def lars_ratio(norms, trust, eps, adaptive):
    pn, gn = math.sqrt(norms[0]), math.sqrt(norms[1])
    return trust * pn / (gn + eps) if (adaptive and pn > 0 and gn > 0) else 1.0


def lars_step(p, g, buf, lr, momentum, wd, trust, eps, first, adaptive, norms=None):
    """contrast/lars.py around SGD momentum for one tensor: the trust ratio trust |p| / (|g'| + eps) scales g' = g + wd p only in an
    adaptive group and only when both norms are > 0.  norms: (sum p^2, sum g'^2) to take the ratio from, default lars_norms."""
    ratio = lars_ratio(lars_norms(p, g, wd) if norms is None else norms, trust, eps, adaptive)
    return sgd_step(p, g, buf, lr, momentum, wd, first, ratio)


def ema(key, query, m):
    return key.double() * m + query.double() * (1.0 - m)


def tick_adam(t, b1, b2):
    return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)


def tick_ema(k, m0, K):
    return 1.0 - (1.0 - m0) * (math.cos(math.pi * k / K) + 1.0) / 2.0


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def _s(x):
    return torch.tensor(float(x), dtype=F32)


def _tree64(x):
    """wave_sum over the last axis (64 lanes): xor 1, 2, 4, 8, 16, 32 - adjacent pairs, six times"""
    for _ in range(6):
        x = x.reshape(*x.shape[:-1], -1, 2)
        x = x[..., 0] + x[..., 1]
    return x.squeeze(-1)


def _block256(acc):
    """[..., 256] per-thread sums -> one value per block: four wave sums, added in wave order"""
    w = _tree64(acc.reshape(*acc.shape[:-1], 4, 64))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def emulate_norms(p, g, wd, mutation=None):
    """mt_norms_kernel + mt_norms_fold_kernel in fp32 on the CPU, in their summation order: a thread adds its 8 x 4 elements of a
    chunk in index order, a block folds 4 wave trees, the fold kernel's thread b adds partials b, b + 256, .. -> fp32 [2]"""
    n = p.numel()
    if n == 0:
        return torch.zeros(2, dtype=F32)
    nb = (n + CHUNK - 1) // CHUNK
    pp = torch.zeros(nb * CHUNK, dtype=F32)
    gg = torch.zeros(nb * CHUNK, dtype=F32)
    pp[:n], gg[:n] = p.reshape(-1).float().cpu(), g.reshape(-1).float().cpu()
    gr = gg if mutation == "norm_without_decay" else gg + _s(wd) * pp
    out = []
    for x in (pp, gr):
        sq = (x * x).view(nb, 8, 256, 4)
        acc = torch.zeros(nb, 256, dtype=F32)
        for k in range(8):
            for e in range(4):
                acc = acc + sq[:, k, :, e]
        part = _block256(acc)                                   # [nb]
        rows = (nb + 255) // 256
        pad = torch.zeros(rows * 256, dtype=F32)
        pad[:nb] = part
        acc = torch.zeros(256, dtype=F32)
        for r in range(rows):
            acc = acc + pad[r * 256:(r + 1) * 256]
        out.append(_block256(acc))
    return torch.stack(out)


MUTATIONS = ["b2", "eps_before_c2", "no_decay", "first_ignored", "norm_without_decay", "ratio_at_zero_p", "tail_unwritten", "ema_swapped"]


def emulate_fp32(kind, p, g, m=None, v=None, *, lr=0.0, b1=0.0, b2=0.0, eps=0.0, wd=0.0, c1=1.0, c2=1.0, first=False, trust=0.0,
                 adaptive=False, mutation=None):
    """multi_tensor_kernel on one tensor in torch fp32 on the CPU, operation by operation.  kind: "adam" | "sgd" | "lars" | "ema"
    (ema: p = key, g = query, b1 = momentum; sgd / lars: b1 = momentum, m = buffer).  -> {"p", "m", "v", "norms"} (fp32; those the
    kind writes).  mutation: one of MUTATIONS - a deliberately wrong kernel, for the sensitivity tests of the comparator."""
    assert mutation is None or mutation in MUTATIONS
    p, g = p.float().cpu(), g.float().cpu()
    m = None if m is None else m.float().cpu()
    v = None if v is None else v.float().cpu()
    if mutation == "b2":
        b2 = 0.9985
    if mutation == "no_decay":
        wd = 0.0
    if mutation == "first_ignored":
        first = False
    if mutation == "ema_swapped" and kind == "ema":
        b1 = f32(1.0 - b1)
    lr_, b1_, b2_, eps_, wd_, c1_, c2_ = (_s(x) for x in (lr, b1, b2, eps, wd, c1, c2))
    one = _s(1.0)
    out = {}
    if kind == "adam":
        gr = g + wd_ * p
        m1 = b1_ * m + (one - b1_) * gr
        v1 = b2_ * v + (one - b2_) * gr * gr
        denom = (v1.sqrt() + eps_) / c2_ if mutation == "eps_before_c2" else v1.sqrt() / c2_ + eps_
        p1 = p - (lr_ / c1_) * (m1 / denom)
        out = {"p": p1, "m": m1, "v": v1}
    elif kind in ("sgd", "lars"):
        ratio = one
        if kind == "lars" and adaptive:
            norms = emulate_norms(p, g, wd, mutation)
            out["norms"] = norms
            pn, gn = norms[0].sqrt(), norms[1].sqrt()
            if (pn > 0 or mutation == "ratio_at_zero_p") and gn > 0:
                ratio = _s(trust) * pn / (gn + eps_)
        gr = (g + wd_ * p) * ratio
        m1 = gr if first else b1_ * m + gr
        p1 = p - lr_ * (m1 if b1 != 0 else gr)
        out.update({"p": p1, "m": m1})
    elif kind == "ema":
        out = {"p": p * b1_ + g * (one - b1_)}
    else:
        raise ValueError(kind)
    if mutation == "tail_unwritten" and p.numel() % 4 == 1:
        for key, old in (("p", p), ("m", m), ("v", v)):
            if key in out and old is not None:
                out[key] = out[key].clone()
                out[key].view(-1)[-1] = old.view(-1)[-1]
    return out


# ------------------------------------------------------------------------------------------------------------------ comparator
def _units(delta, scale):
    """max over the elements of |delta| / (u scale); scale 0 wants delta 0"""
    if delta.numel() == 0:
        return 0.0
    delta, scale = delta.abs(), scale.abs()
    inf = torch.full_like(delta, float("inf"))
    r = torch.where(scale > 0, delta / (U * scale.clamp_min(1e-300)), torch.where(delta > 0, inf, torch.zeros_like(delta)))
    r = torch.where(torch.isnan(r), inf, r)
    return float(r.max())


def reference(kind, p, g, m=None, v=None, *, lr=0.0, b1=0.0, b2=0.0, eps=0.0, wd=0.0, c1=1.0, c2=1.0, first=False, trust=0.0,
              adaptive=False):
    """the float64 step of `kind` with emulate_fp32's arguments -> {"p", "m", "v", "norms"} in float64"""
    if kind == "adam":
        p1, m1, v1 = adam_step(p, g, m, v, lr, b1, b2, eps, wd, c1, c2)
        return {"p": p1, "m": m1, "v": v1}
    if kind == "sgd":
        p1, m1 = sgd_step(p, g, m, lr, b1, wd, first)
        return {"p": p1, "m": m1}
    if kind == "lars":
        norms = lars_norms(p, g, wd)
        p1, m1 = lars_step(p, g, m, lr, b1, wd, trust, eps, first, adaptive, norms)
        out = {"p": p1, "m": m1}
        if adaptive:
            out["norms"] = norms
        return out
    if kind == "ema":
        return {"p": ema(p, g, b1)}
    raise ValueError(kind)


def compare(kind, got, p, g, m=None, v=None, **sc):
    """Hold what a kernel (or its emulation) wrote - got = {"p", "m", "v", "norms"}, the ones `kind` writes - against the float64 step
    from the same fp32 inputs.  -> {metric: units}; every element is compared."""
    ref = reference(kind, p, g, m, v, **sc)
    dev = p.device
    pd, gd = p.double(), g.double()
    b1, wd = sc.get("b1", 0.0), sc.get("wd", 0.0)
    res = {}
    if kind == "ema":
        res["upd"] = _units(got["p"].to(dev).double() - ref["p"], (b1 * pd).abs() + ((1.0 - b1) * gd).abs())
        return res
    gr = gd + wd * pd
    if kind == "adam":
        res["m"] = _units(got["m"].to(dev).double() - ref["m"], (b1 * m.double()).abs() + ((1.0 - b1) * gr).abs())
        res["v"] = _units(got["v"].to(dev).double() - ref["v"], ref["v"])
    else:
        ratio = lars_ratio(ref["norms"], sc.get("trust", 0.0), sc.get("eps", 0.0), True) if "norms" in ref else 1.0
        res["m"] = _units(got["m"].to(dev).double() - ref["m"],
                          (gr * ratio).abs() if sc.get("first") else (b1 * m.double()).abs() + (gr * ratio).abs())
        if "norms" in ref:
            res["norm"] = _units(torch.as_tensor(got["norms"]).double().cpu().reshape(2) - torch.tensor(ref["norms"], dtype=F64),
                                 torch.tensor(ref["norms"], dtype=F64))
    upd_ref = pd - ref["p"]
    res["upd"] = _units((pd - got["p"].to(dev).double()) - upd_ref, upd_ref.abs() + ref["p"].abs())
    return res


# ------------------------------------------------------------------------------------------------------------------ regimes
ADAM_T = {"warm": 1000}          # the step the bias corrections belong to (default: the first)


def scalars(kind, regime, momentum=0.9, first=False, adaptive=True):
    """The scalars of one launch of `kind` under `regime`, rounded as the C ABI receives them.  Adam's "unit" has no weight decay:
    from a zero state the scale of `m` and `v` is g' = g + wd p alone, which cancels where |g| happens to be ~ wd |p|, and the
    largest of 85 000 such ratios is a property of the sample (57 u and 2449 u for two seeds), not of the arithmetic; the decay
    term is pinned where something else carries the scale (warm, zero_g: the state; small_p: g)."""
    if kind == "adam":
        c1, c2 = tick_adam(ADAM_T.get(regime, 1), 0.9, 0.999)
        return dict(lr=f32(1e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), wd=0.0 if regime == "unit" else f32(1e-2), c1=f32(c1),
                    c2=f32(c2))
    if kind == "sgd":
        return dict(lr=f32(0.01), b1=f32(momentum), wd=f32(1e-4), first=first)
    if kind == "lars":
        return dict(lr=f32(0.5), b1=f32(momentum), wd=f32(1e-5), eps=f32(1e-8), trust=f32(1e-3), first=first, adaptive=adaptive)
    if kind == "ema":
        return dict(b1=f32(0.99))
    raise ValueError(kind)


def values(regime, n, seed, lr=1e-3):
    """fp32 CPU inputs (p, g, m, v) of n elements: see the regimes in tests/test_hip_optim_contract.py.  The state is non-zero in
    "warm" and "zero_g" (there a buffer that a first step should overwrite holds something) and zero elsewhere: where the update is
    all there is to p ("small_p", "zero_p"), b1 m0 + (1 - b1) g' from an unrelated m0 cancels in some elements, and `upd`, whose
    scale is the update itself, would measure that cancellation instead of the arithmetic."""
    gen = torch.Generator().manual_seed(1000003 * seed + n)
    r = lambda: torch.randn(n, generator=gen, dtype=F32)  # noqa: E731
    p, g, m, v = r(), r(), 0.1 * r(), (0.1 * r()) ** 2 + 1e-6 * torch.rand(n, generator=gen, dtype=F32)
    if regime not in ("warm", "zero_g"):
        m, v = torch.zeros(n), torch.zeros(n)
    if regime == "small_p":
        p = p * (1e-4 * lr)
    if regime == "tiny_g":
        g = g * 1e-8
    if regime == "zero_g":
        g = torch.zeros(n)
    if regime == "zero_p":
        p = torch.zeros(n)
    return p, g, m, v


def cases():
    """[(kind, label, regime, options of scalars())]: the launches both test files run.  label = the regime, or what else the case
    is about; BOUND of tests/test_hip_optim_contract.py is keyed by (kind, metric, label); first = True / False share a key."""
    out = [("adam", r, r, {}) for r in REGIMES]
    for kind in ("sgd", "lars"):
        for r in REGIMES:
            if r != "tiny_g":             # (a gradient below the decay term: nothing the other regimes do not do)
                out += [(kind, r, r, dict(first=f)) for f in (True, False)]
        out += [(kind, "mom0", "warm", dict(momentum=0.0, first=f)) for f in (True, False)]
    out += [("lars", "nonadaptive", "warm", dict(adaptive=False, first=f)) for f in (True, False)]
    out.append(("ema", "unit", "unit", {}))
    return out


def list_counts(kind):
    """list lengths around the 48 tensors of a launch; LARS also 96: a full second launch whose norms stay readable"""
    return (1, 47, 48, 49, 96, 97) if kind == "lars" else (1, 47, 48, 49, 97)


def list_sizes(n):
    """n tensors, the multi-chunk ones not first"""
    cyc = [3, 1, 8193, 5, 4, 1025, 16391, 1023, 8191, 1024, 8192, 3 * 8192]
    return [cyc[i % len(cyc)] for i in range(n)]


def list_case(kind, count):
    """-> (regime, scalars, [(p, g, m, v)] of the `count` tensors): a later step from a non-zero state (EMA: "unit")"""
    regime = "unit" if kind == "ema" else "warm"
    sc = scalars(kind, regime, first=False) if kind in ("sgd", "lars") else scalars(kind, regime)
    return regime, sc, [values(regime, n, count + i, lr=sc.get("lr", 1e-3)) for i, n in enumerate(list_sizes(count))]


LARS_BIG_LIST = [5, 8193, LARS_BIG, 1025, 3 * 8192]          # the 300-chunk tensor neither first nor last


def big_case():
    """-> (scalars, [(p, g, m, v)]) of the LARS launch over LARS_BIG_LIST ("warm": a later step from a non-zero buffer)"""
    return scalars("lars", "warm", first=False), [values("warm", n, 77) for n in LARS_BIG_LIST]


def case_id(c):
    return f"{c[0]}-{c[1]}" + ("".join(f"-{k}{int(v) if isinstance(v, bool) else v}" for k, v in c[3].items() if k == "first"))


# ------------------------------------------------------------------------------------------------------------------ trajectories
def trajectory_error(ps, refs, inits):
    """max |p - p64| / max |p64 - p_initial| over the parameters: error over distance moved"""
    return max(float((p.detach().double().cpu() - r.double()).abs().max() / (r.double() - i.double()).abs().max())
               for p, r, i in zip(ps, refs, inits))


ADAM_TRAJ = dict(shapes=[(33, 17), (8193,), (5,), (3 * 8192 + 7,)], steps=50, lr=1e-3, wd=1e-2, sits_out=(1, range(10, 20)), seed=11)


def adam_traj_inputs():
    gen = torch.Generator().manual_seed(ADAM_TRAJ["seed"])
    p0 = [torch.randn(*s, generator=gen) for s in ADAM_TRAJ["shapes"]]
    idx, when = ADAM_TRAJ["sits_out"]
    grads = [[None if (i == idx and t in when) else torch.randn(*s, generator=gen) * (1 + i) for i, s in enumerate(ADAM_TRAJ["shapes"])]
             for t in range(ADAM_TRAJ["steps"])]
    return p0, grads


def run_optimizer(make, p0, grads, dtype=F32, device="cpu"):
    """step `make(params)` through `grads` from p0 -> final parameters"""
    ps = [p.to(device=device, dtype=dtype).clone().requires_grad_(True) for p in p0]
    opt = make(ps)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(device=device, dtype=dtype)
        opt.step()
    return [p.detach() for p in ps]


def adam_traj_reference():
    """-> (p0, grads, float64 torch.optim.Adam result, drift of fp32 torch.optim.Adam on the CPU against it)"""
    p0, grads = adam_traj_inputs()
    mk = lambda ps: torch.optim.Adam(ps, ADAM_TRAJ["lr"], weight_decay=ADAM_TRAJ["wd"])  # noqa: E731
    p64 = run_optimizer(mk, p0, grads, F64)
    p32 = run_optimizer(mk, p0, grads, F32)
    return p0, grads, p64, trajectory_error(p32, p64, p0)


LARS_TRAJ = dict(steps=20, lr=1.0, momentum=0.9, wd=1e-5, trust=1e-3, eps=1e-8, seed=12)


def lars_traj_module():
    """one parameter of more than 3 chunks, 1-D parameters (no decay, no trust ratio), a small matrix"""
    torch.manual_seed(LARS_TRAJ["seed"])
    return torch.nn.Sequential(torch.nn.Linear(160, 160), torch.nn.LayerNorm(160), torch.nn.Linear(160, 7, bias=False))


def lars_traj_reference():
    """-> (names, p0, grads, float64 result, drift of the fp32 torch restatement - oracle.lars_sgd_step on the CPU - against it), the
    groups as add_weight_decay makes them: 1-D parameters without decay and trust ratio"""
    from oracle.stswin_oracle import lars_sgd_step
    net = lars_traj_module()
    names = [n for n, _ in net.named_parameters()]
    p0 = [p.detach().clone() for _, p in net.named_parameters()]
    gen = torch.Generator().manual_seed(LARS_TRAJ["seed"] + 1)
    grads = [[torch.randn(p.shape, generator=gen) * 0.1 for p in p0] for _ in range(LARS_TRAJ["steps"])]
    c = LARS_TRAJ
    p64 = [p.double().clone() for p in p0]
    buf64 = [None] * len(p0)
    p32 = [p.clone() for p in p0]
    buf32 = [None] * len(p0)
    for t, gs in enumerate(grads):
        for i, g in enumerate(gs):
            adaptive = p0[i].dim() != 1
            wd = c["wd"] if adaptive else 0.0
            b = torch.zeros_like(p64[i]) if buf64[i] is None else buf64[i]
            p64[i], buf64[i] = lars_step(p64[i], g, b, c["lr"], c["momentum"], wd, c["trust"], c["eps"], t == 0, adaptive)
            one_p, one_b = [p32[i]], [buf32[i]]
            lars_sgd_step(one_p, [g], one_b, c["lr"], c["momentum"], wd, adaptive, c["trust"], c["eps"])
            buf32[i] = one_b[0]
    return names, p0, grads, p64, trajectory_error(p32, p64, p0)
