"""fp64 references with a per-element error model for the likelihood kernels of csrc/entropy.hip (a plain module, not a conftest).
Used by tests/test_entropy_ref_cpu.py (no GPU) and tests/test_gpu_entropy_parity.py.

Reference values.  ``gmm_chain`` (GaussianConditional, the mixture) and ``eb_chain`` (EntropyBottleneck, its aux loss) restate a kernel's
arithmetic in fp64 torch, node for node, on exactly the operands the kernel receives (storage-rounded, widened to fp64).  With every slot at
zero they ARE oracle.hesic_oracle's gc_forward / gmm_forward / eb_forward / eb_aux_loss and, for the hand-written backward formulas, their fp64
autograd (tests/test_entropy_ref_cpu.py holds both to 1e-10).

Error unit.  Every value the kernel rounds passes through a slot  x (1 + d_j) + e_j  (``Slots``), d_j and e_j zero tensors of the value's
shape.  The chains are elementwise per latent, so one backward of out.sum() yields d out_e / d d_{j,e} for every element at once and

    unit_e = 2^-24 sum_j k_j |d out_e / d d_{j,e}|  +  2^-126 sum_j |d out_e / d e_{j,e}|.

k_j is the ulp count of the operation that produced node j (constants below, each with its source); the second sum is the absolute error
of a result that leaves fp32's normal range (the hardware exp2 / rcp and a multiply may flush it: < 2^-126 per node).  Nothing is fitted:
no constant comes from a GPU run of these kernels.

Bars.  Elementwise outputs: |got_e - ref_e| <= unit_e + store_e (c = 1: the unit is a worst-case count), store_e = u |ref_e| + h for a
16-bit destination.  Where unit_e == 0 the value must be exactly the reference: the likelihood at the floor is exactly lik_bound (the operands
keep every unclamped likelihood a factor 2 away from it), a masked gradient is exactly 0, dy in round mode is exactly 0.  The scale mask's
``dsk < 0`` clause: an element below the scale bound whose reference |dsk| lies inside its own unit keeps that unit (either decision passes);
every other masked element has unit 0.  dweights (a sum over the pixels of one (batch, component, channel) through float atomics):
bar = C_BAR sqrt(n) 2^-24 S + sum_p unit_p, S = sum_p |g_p pk_p|, n = HW (C_BAR = 8: an fp32 sum in any order, tests/conv_grad_ref.py).
"""
import functools
import math

import torch

C_BAR = 8.0
U24 = 2.0 ** -24
TINY = 2.0 ** -126
# ulp counts, in units of 2^-24 relative
K_ARITH = 1.0       # + - * fma and division by "/": correctly rounded is 1/2.  A product with a constant that is itself an fp32 rounding of
#                     the exact one (1/sqrt 2, 1/sqrt(2 pi), log2(e)/2) spends the other half on the constant.
K_RCP = 1.0         # __builtin_amdgcn_rcpf: v_rcp_f32, 1 ulp (CDNA ISA guide, "V_RCP_F32 ... 1ULP accuracy")
K_EXP2 = 1.0        # __builtin_amdgcn_exp2f: v_exp_f32, 1 ulp (same table)
# ocml: no ulp bound is documented with the installed ROCm; these are the OpenCL full-profile single-precision bounds OCML is built to meet
# (OpenCL C specification, "Relative error as ULPs")
K_ERFC, K_TANH, K_EXP, K_LOG1P = 16.0, 5.0, 3.0, 2.0
# erfc_fast (csrc/entropy.hip), a >= 0:  erfc(a) = Q(p) * rcp(2 a + 1) * exp2(-log2(e) a^2), p = (a - 2) rcp(a + 2), a^2 split into its rounded
# value and the fma remainder.  The chain restates it node for node; the one node that is not a single operation is the degree-10 Horner
# form Q against erfcx(a) (1 + 2 a).  derive_erfc_fast() evaluates it in emulated fp32 on a dense grid of a in [0, 10.2] (fit error
# included): K_POLY is that worst relative error in units of 2^-24 rounded up, plus the one hardware ulp it contains (the v_rcp_f32 in p, which
# the emulation rounds correctly).  The same function reports the whole of erfc_fast as ONE relative constant (K_ERFC_FAST_WHOLE, with its three
# hardware ulps); it is not used in a bar, because it is set by the far tail, where the rounding of -log2(e) a^2 (|.| up to 150) is
# multiplied by ln 2 |.| -- the chain's slot on that node carries exactly this factor per element.  tests/test_entropy_ref_cpu.py asserts both.
K_POLY = 4.0 + 1.0
K_ERFC_FAST_WHOLE = 62.0 + 3.0
LOG2E = 1.0 / math.log(2.0)

SQRT1_2 = 2.0 ** -0.5
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)
HALF_LOG2E = 0.5 / math.log(2.0)
SCALE_BOUND = float(torch.tensor(0.11, dtype=torch.float32))
LIK_BOUND = float(torch.tensor(1e-9, dtype=torch.float32))
# 16-bit storage: (u, h): |round(x) - x| <= u |x| + h.  h = half the subnormal step of the format.
FMT = {torch.bfloat16: (2.0 ** -8, 2.0 ** -134), torch.float16: (2.0 ** -11, 2.0 ** -25), torch.float32: (0.0, 0.0), None: (0.0, 0.0)}
CHUNK = 1 << 16          # latents per pass of a chain: bounds the memory of the slots


# ====================================================================================================================== slots
class Slots:
    """Records a multiplicative and an additive slot at every rounded node; ``unit`` turns them into the per-element bound."""

    def __init__(self):
        self.items = []

    def __call__(self, x, k=K_ARITH):
        d = torch.zeros_like(x, requires_grad=True)
        e = torch.zeros_like(x, requires_grad=True)
        self.items.append((d, e, float(k)))
        return x * (1 + d) + e

    def add(self, a, b):
        """a + b, exact (no slot) where either operand is exactly 0."""
        both = ((a.detach() != 0) & (b.detach() != 0)).to(a.dtype)
        d = torch.zeros_like(both, requires_grad=True)
        e = torch.zeros_like(both, requires_grad=True)
        self.items.append((d, e, K_ARITH))
        return (a + b) * (1 + d * both) + e * both

    def unit(self, out):
        leaves = [d for d, _, _ in self.items] + [e for _, e, _ in self.items]
        grads = torch.autograd.grad(out.sum(), leaves, retain_graph=True, allow_unused=True)
        n = len(self.items)
        u = torch.zeros_like(out)
        for j, g in enumerate(grads):
            if g is None:
                continue
            a = g.detach().abs()
            while a.dim() > out.dim():            # a per-component node feeding a per-latent output: its components' shares add up
                a = a.sum(0)
            assert a.shape == out.shape, "a shared node may not feed a per-component output: expand it before its slot"
            u += a * (self.items[j][2] * U24 if j < n else TINY)
        return u.detach()


class NoSlots:
    """The chain without slots: plain fp64 (or, in another dtype, that dtype's own evaluation)."""
    items = ()

    def __call__(self, x, k=K_ARITH):
        return x

    def add(self, a, b):
        return a + b

    def unit(self, out):
        return torch.zeros_like(out)


# ================================================================================================================== erfc_fast
ERFC_FAST_COEF = (5.535401624402612e-05, -0.0003277268339344692, -0.0012812873942078364, 0.001231548543911547, 0.008647743766865298,
                  -0.008028522672854756, -0.054206538593428145, 0.16405084760016128, -0.1660312591225932, -0.0927638072951173,
                  1.2769783903081213)


def erfc_fast_model(a, dtype, parts=False):
    """erfc_fast of csrc/entropy.hip for a >= 0 (fp64 tensor), evaluated in ``dtype``: the same coefficients, the same (a - 2) / (a + 2)
    argument, the same split a^2.  fp32: every operation rounded once (an fma is formed in fp64 and rounded).  ``parts``: (erfc, Q)."""
    f = (lambda t: t.to(torch.float32).double()) if dtype == torch.float32 else (lambda t: t)
    c = [float(f(torch.tensor(v, dtype=torch.float64))) for v in ERFC_FAST_COEF]
    log2e = float(f(torch.tensor(LOG2E, dtype=torch.float64)))
    a = f(a)
    p = f(f(a - 2.0) * f(1.0 / f(a + 2.0)))
    q = torch.full_like(a, c[0])
    for v in c[1:]:
        q = f(q * p + v)
    s2 = f(a * a)
    el = f(a * a - s2)
    ex = f(torch.exp2(f(-log2e * s2)))
    ex = f(-el * ex + ex)
    ec = f(f(q * f(1.0 / f(2.0 * a + 1.0))) * ex)
    return (ec, q) if parts else ec


def derive_erfc_fast(n=2_000_001):
    """On a dense grid of fp32 values a in [0, 10.2], in units of 2^-24 relative: (fit, whole, poly).  fit: the kernel's form evaluated in
    fp64 against erfc(a) (the fit error alone); whole: the same in emulated fp32,  (|err| - 2^-126) / erfc(a)  (beyond a = 9.3 the result
    leaves fp32's normal range); poly: the Horner form Q in emulated fp32 against erfcx(a) (1 + 2 a)."""
    a = torch.linspace(0.0, 10.2, n, dtype=torch.float64).to(torch.float32).double()
    ref = torch.erfc(a)
    fit = float(((erfc_fast_model(a, torch.float64) - ref).abs() / (U24 * ref)).max())
    ec, q = erfc_fast_model(a, torch.float32, parts=True)
    whole = float((((ec - ref).abs() - TINY).clamp_min(0) / (U24 * ref)).max())
    qref = torch.special.erfcx(a) * (1.0 + 2.0 * a)
    poly = float(((q - qref).abs() / (U24 * qref)).max())
    return fit, whole, poly


# ================================================================================================================ storage bars
def storage(ref, dtype, times=1.0):
    u, h = FMT[dtype]
    return times * (u * ref.abs() + h) if u else torch.zeros_like(ref)


def check(R, got, name=""):
    """(ok, ratio, message) of ``got`` against R = {"ref", "unit"[, "store"]}: |got - ref| <= unit + store for EVERY element (no element is
    left out); ratio = max_e (|err_e| - store_e) / unit_e over the elements with a unit, inf if an element without one is not exact."""
    ref, unit = R["ref"], R["unit"]
    got = got.detach().double().cpu().reshape(ref.shape)
    store = R.get("store")
    store = torch.zeros_like(ref) if store is None else store
    err = (got - ref).abs()
    live = unit > 0
    ratio = float(((err - store).clamp_min(0)[live] / unit[live]).max()) if bool(live.any()) else 0.0
    bad = ~(err <= unit + store)                      # NaN counts as a miss
    if bool((bad & ~live).any()):
        ratio = math.inf
    msg = ""
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        worst = tuple(int(i) for i in idx[torch.argmax(torch.nan_to_num(err - unit - store, nan=1e300)[bad])])
        msg = (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside their bar; worst at {worst}: got {float(got[worst]):.9g} "
               f"ref {float(ref[worst]):.9g} bar {float((unit + store)[worst]):.3g}; first index per dim {[int(i) for i in idx.min(0).values]} "
               f"last {[int(i) for i in idx.max(0).values]}; exact-required elements hit {int((bad & ~live).sum())}")
    return not bool(bad.any()), ratio, msg


def changed_share(R, mutant):
    """(share of the changed elements that leave their bar, number of changed elements) of a mutated fp64 result."""
    ref, unit = R["ref"], R["unit"]
    store = R.get("store")
    store = torch.zeros_like(ref) if store is None else store
    mutant = mutant.double().reshape(ref.shape)
    changed = mutant != ref
    out = (mutant - ref).abs() > unit + store
    n = int(changed.sum())
    return (float((out & changed).sum()) / n if n else 0.0), n


# ============================================================================================= Gaussian / Gaussian mixture: cases
# st: storage of y / scales / means / noise ("f32" | "h16": the library's 16-bit format); mode: "round" | "noise"; umq: means in the quantiser
# (GaussianConditional, K == 1); gy: a gradient arrives on y_hat; wide: scales | means are the two halves of one (B, HW, 2 K M) tensor
# (pixel stride 2 K M, s_c_off 0, m_c_off K M); f32in: fp32 operands with y_hat stored as "h16" | "f32" (hesic_gmm_forward_f32in); bwd: the case
# also runs the backward; big: kept out of the CPU suite's per-case loops (the GPU test runs it).  Derivations of the shapes from the launch
# code are in tests/test_gpu_entropy_parity.py, next to each case.
def _g(B, H, W, M, K, st, mode="round", umq=False, gy=False, wide=False, f32in=None, bwd=False, big=False, means=True):
    return dict(B=B, H=H, W=W, M=M, K=K, st=st, mode=mode, umq=umq, gy=gy, wide=wide, f32in=f32in, bwd=bwd, big=big, means=means,
                weights=K > 1)


GMM = {
    # non-pair forward (gmm_fwd_kernel<float> / <h16_t>) and the run-time-K backward (gmm_bwd_kernel<.., 0>)
    "k1_umq_f32": _g(2, 5, 7, 65, 1, "f32", umq=True, gy=True, bwd=True),
    "k1_plain_h16": _g(2, 5, 7, 65, 1, "h16", means=False),
    "k2_h16": _g(2, 5, 7, 65, 2, "h16", mode="noise", gy=True, bwd=True),
    "k3_f32": _g(2, 2, 3, 65, 3, "f32", mode="noise", gy=True, bwd=True),
    "k3_h16": _g(2, 5, 7, 65, 3, "h16", bwd=True),
    "k5_f32": _g(2, 5, 7, 65, 5, "f32", bwd=True),
    "k8_h16": _g(2, 5, 7, 65, 8, "h16", mode="noise", bwd=True),
    "k5_oddm_h16": _g(2, 5, 7, 65, 5, "h16"),
    "k1_trip2_f32": _g(1, 90, 90, 65, 1, "f32", umq=True, big=True),
    # pair forward (gmm_fwd_pair_kernel<1 / 5>) and the compile-time-K backward (gmm_bwd_kernel<h16_t, 1 / 5>)
    "pair_k5_m16": _g(2, 5, 7, 16, 5, "h16", bwd=True),
    "pair_k5_m192": _g(2, 5, 7, 192, 5, "h16", mode="noise", gy=True, bwd=True),
    "pair_k1_m16_umq": _g(2, 5, 7, 16, 1, "h16", umq=True, gy=True, bwd=True),
    "pair_k1_m192_noise": _g(2, 16, 17, 192, 1, "h16", mode="noise", umq=True, gy=True, bwd=True),
    "pair_k5_m65_bwd": _g(2, 5, 7, 65, 5, "h16", mode="noise", gy=True, bwd=True),
    "pair_k5_wide": _g(2, 5, 7, 16, 5, "h16", wide=True, bwd=True),
    "pair_k1_wide_umq": _g(2, 5, 7, 192, 1, "h16", umq=True, wide=True),
    "pair_k1_trip2": _g(1, 100, 164, 64, 1, "h16", umq=True, big=True),
    "f32in_k5_h16": _g(2, 5, 7, 16, 5, "f32", f32in="h16"),
    "f32in_k1_f32": _g(2, 5, 7, 192, 1, "f32", umq=True, f32in="f32"),
    "f32in_k5_wide_f32": _g(2, 5, 7, 16, 5, "f32", wide=True, f32in="f32"),
    # pix_per_block of hesic_gmm_backward: 8 with HW % 8 = 5 and HW % 4 = 1, and the cap 64 with a remainder of 16 pixels
    "bwd_k1_ppb8": _g(2, 35, 23, 192, 1, "h16", mode="noise", umq=True, gy=True, bwd=True, big=True),
    "bwd_k1_cap64": _g(2, 100, 164, 65, 1, "h16", umq=True, gy=True, bwd=True, big=True),
}
GMM_SMALL = [n for n, c in GMM.items() if not c["big"]]


def pix_per_block(B, HW, M):
    """hesic_gmm_backward's choice, restated."""
    other = ((M + 63) // 64) * B
    want = (1024 + other - 1) // other
    ppb = (HW + want - 1) // want
    ppb = (ppb + 3) // 4 * 4
    return max(4, min(64, ppb))


def fast_path(case, what, is16=True):
    """True where the launch code takes the erfc_fast / rcp / exp2 form: the pair forward, and the backward with K known at compile time."""
    c = GMM[case] if isinstance(case, str) else case
    if what == "fwd":
        if c["f32in"]:
            return True
        return c["st"] == "h16" and c["K"] in (1, 5) and c["M"] % 2 == 0
    return c["st"] == "h16" and c["K"] in (1, 5)


def _sdt(c, h16):
    return torch.float32 if c["st"] == "f32" else h16


def _grid(gen, shape, lo, hi):
    return torch.round((torch.rand(shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo) * 16) / 16


def _neighbours(dtype):
    """The storage type's values around 0.11f: two below, two at or above (fp32: 0.11f itself and its neighbours)."""
    it = torch.int32 if dtype == torch.float32 else torch.int16
    b = torch.tensor([SCALE_BOUND], dtype=torch.float32).to(dtype)
    bits = b.view(it).to(torch.int64) + torch.arange(-2, 3)
    return bits.to(it).view(dtype).double()


@functools.lru_cache(maxsize=None)
def gmm_operands(name, h16=torch.bfloat16):
    """The operands of a case in the kernel's layout, fp64 holding storage-exact values: y, noise, gy (B, HW, M); scales, means
    (B, HW, K, M); weights (B, K, M) fp32-exact; g (B, HW, M) fp32-exact."""
    c = GMM[name]
    B, HW, M, K = c["B"], c["H"] * c["W"], c["M"], c["K"]
    sdt = _sdt(c, h16)
    gen = torch.Generator().manual_seed(1000 + sorted(GMM).index(name))
    N = B * HW * M
    y = _grid(gen, (N,), -11, 11)
    mu = _grid(gen, (N, K), -4, 4) if c["means"] else torch.zeros((N, K), dtype=torch.float64)
    sc = torch.exp(torch.rand((N, K), generator=gen, dtype=torch.float64) * math.log(64 / 0.02) + math.log(0.02))
    # ~5 % of the latents far in every component's tail: below the likelihood floor
    far = torch.rand((N,), generator=gen) < 0.06
    sc[far] = torch.exp(torch.rand((int(far.sum()), K), generator=gen, dtype=torch.float64) * math.log(0.3 / 0.02) + math.log(0.02))
    y[far] = torch.where(y[far] >= 0, 1.0, -1.0) * _grid(gen, (int(far.sum()),), 8, 11)
    sc = sc.to(sdt).double()
    nb = _neighbours(sdt)
    idx = torch.arange(0, N * K, 11)
    sc.view(-1)[idx] = nb[torch.arange(idx.numel()) % nb.numel()]
    noise = _grid(gen, (N,), -0.5, 0.5) if c["mode"] == "noise" else None
    # exact ties of the quantiser: y - mu (or y) = +-0.5, +-1.5, +-2.5
    if c["mode"] == "round":
        ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], dtype=torch.float64)
        ti = torch.arange(3, N, 37)
        y[ti] = ties[torch.arange(ti.numel()) % 6] + (mu[ti, 0] if c["umq"] else 0.0)
    w = None
    if c["weights"]:
        w = torch.softmax(2.0 * torch.randn((B, K, M), generator=gen, dtype=torch.float64), 1).to(torch.float32).double()
    g = torch.randn((N,), generator=gen, dtype=torch.float64).to(torch.float32).double()
    gy = _grid(gen, (N,), -2, 2) if c["gy"] else None
    o = dict(y=y, mu=mu, sc=sc, noise=noise, w=w, g=g, gy=gy)
    # keep every unclamped likelihood a factor 2 away from the bound: an offender moves onto its first mean (a likelihood far above it)
    for _ in range(8):
        L = _gmm_lik_plain(c, o)
        off = (L > LIK_BOUND / 2) & (L < LIK_BOUND * 2)
        if not bool(off.any()):
            break
        o["y"][off] = torch.round(mu[off, 0])
    shp = (B, HW, M)
    out = dict(y=o["y"].reshape(shp), means=mu.reshape(B, HW, M, K).permute(0, 1, 3, 2).contiguous(),
               scales=sc.reshape(B, HW, M, K).permute(0, 1, 3, 2).contiguous(), weights=w, g=g.reshape(shp),
               noise=None if noise is None else noise.reshape(shp), gy=None if gy is None else gy.reshape(shp))
    return out


def _flat(c, ops):
    """(B, HW, [K,] M) operands -> the chain's flat form: per-latent (N,), per-component (K, N)."""
    B, HW, M, K = c["B"], c["H"] * c["W"], c["M"], c["K"]
    N = B * HW * M
    per_k = lambda t: t.permute(2, 0, 1, 3).reshape(K, N)
    w = ops["weights"]
    return dict(y=ops["y"].reshape(N), mu=per_k(ops["means"]), sc=per_k(ops["scales"]),
                w=None if w is None else w.permute(1, 0, 2)[:, :, None, :].expand(K, B, HW, M).reshape(K, N),
                g=ops["g"].reshape(N), noise=None if ops["noise"] is None else ops["noise"].reshape(N),
                gy=None if ops["gy"] is None else ops["gy"].reshape(N))


def _gmm_lik_plain(c, o):
    """Unclamped mixture likelihood of flat (N,) / (N, K) operands (construction only)."""
    y, mu, sc = o["y"], o["mu"], o["sc"]
    if c["mode"] == "noise":
        v = y + o["noise"]
    elif c["umq"]:
        v = torch.round(y - mu[:, 0]) + mu[:, 0]
    else:
        v = torch.round(y)
    a = (v[:, None] - mu).abs()
    s = sc.clamp_min(SCALE_BOUND)
    pk = 0.5 * torch.erfc(-SQRT1_2 * (0.5 - a) / s) - 0.5 * torch.erfc(-SQRT1_2 * (-0.5 - a) / s)
    if o["w"] is not None:
        B, K, M = o["w"].shape
        pk = pk * o["w"].permute(0, 2, 1)[:, None].expand(B, y.numel() // (B * M), M, K).reshape(-1, K)
    return pk.sum(1)


# ============================================================================================= Gaussian / Gaussian mixture: chain
def gmm_chain(c, f, R, fast, backward, dtype=torch.float64, mut=(), emulate=None):
    """The kernels' arithmetic on flat operands ``f`` (``_flat``), every rounded node through ``R``.  fast: the erfc_fast / rcp / exp2 form.
    Returns a dict of graph tensors: v, L (unclamped), and with ``backward`` the unmasked dsk, keep (scale mask), dmu, dy, and the dweights
    terms (K, N).  ``dtype``: the evaluation's type (fp32: torch's own fp32 evaluation of the same chain).  ``mut``: the CPU test's mutations."""
    cv = lambda t: None if t is None else t.to(dtype)
    y, mu, sraw, w, g, noise, gy = (cv(f[k]) for k in ("y", "mu", "sc", "w", "g", "noise", "gy"))
    K = c["K"]
    sb, lb = torch.tensor(SCALE_BOUND, dtype=dtype), torch.tensor(LIK_BOUND, dtype=dtype)
    rnd = (lambda t: torch.sign(t) * torch.floor(t.abs() + 0.5)) if "round_away" in mut else torch.round
    if noise is not None:
        v = y + noise
    elif c["umq"]:
        v = rnd(y - mu[0]) + mu[0]
    else:
        v = rnd(y)
    s = sraw if "no_clamp" in mut else torch.maximum(sraw, sb)
    df = v - mu
    a = df.abs()
    if fast:
        isc = R(1.0 / s, K_RCP)
        u, l = R((0.5 - a) * isc), R((-0.5 - a) * isc)
    else:
        u, l = R((0.5 - a) / s), R((-0.5 - a) / s)

    def Phi(x):
        z = R(-SQRT1_2 * x)
        if fast:
            aa = z.abs()
            if emulate is not None:                   # the by-design approximation itself (CPU test), no slots
                ec = erfc_fast_model(aa.double(), emulate).to(aa.dtype)
            else:
                q = R(torch.special.erfcx(aa) * (1.0 + 2.0 * aa), K_POLY)
                r = R(1.0 / R(2.0 * aa + 1.0), K_RCP)
                s2 = R(aa * aa)
                el = R(aa * aa - s2)
                ex = R(torch.exp2(R(-LOG2E * s2)), K_EXP2)
                ex = R(ex - el * ex)
                ec = R(R(q * r) * ex)
            return 0.5 * torch.where(z >= 0, ec, R(2.0 - ec))
        return 0.5 * R(torch.erfc(z), K_ERFC)

    pk = R(Phi(u) - Phi(l))
    ks = [k for k in range(K) if not ("drop_component" in mut and k == K - 1)]
    L = None
    for k in ks:
        t = R(pk[k] * w[k]) if w is not None else pk[k]
        L = t if L is None else R.add(L, t)
    out = dict(v=v, L=L, pk=pk)
    if not backward:
        return out
    keep_l = (L.detach() >= lb) | (g < 0)
    if "no_lik_mask" in mut:
        keep_l = torch.ones_like(keep_l)
    if "no_lik_gneg" in mut:
        keep_l = L.detach() >= lb
    ge = torch.where(keep_l, g, torch.zeros_like(g))
    sgn = torch.sign(df)

    def pdf(x):
        if fast:
            return R(INV_SQRT_2PI * R(torch.exp2(R(R(-HALF_LOG2E * x) * x)), K_EXP2))
        return R(INV_SQRT_2PI * R(torch.exp(R((-0.5 * x) * x)), K_EXP))

    gw = R(ge * w) if w is not None else ge.expand_as(u)
    ak, ck = R(gw * pdf(u)), -R(gw * pdf(l))
    if fast:
        dvk, dsk = -R(R(ak + ck) * isc), -R(R(R(ak * u) + R(ck * l)) * isc)
    else:
        dvk, dsk = -R(R(ak + ck) / s), -R(R(R(ak * u) + R(ck * l)) / s)
    keep = (sraw >= sb) | (dsk.detach() < 0)
    if "mask_on_clamped" in mut:
        keep = torch.ones_like(keep)
    if "no_dsk_neg" in mut:
        keep = sraw >= sb
    quant_mu = noise is None and c["umq"]
    dmu = -dvk * sgn
    if quant_mu and "no_dmu_cancel" not in mut:
        dmu = torch.zeros_like(dmu)                  # -x + x: exactly 0
    dv = None
    for k in range(K):
        t = dvk[k] * sgn[k]
        dv = t if dv is None else R.add(dv, t)
    if gy is not None:
        dv = R.add(dv, gy)
        if quant_mu and "no_gy_in_dmeans" not in mut:
            dmu = dmu + gy[None]                     # K == 1; 0 + gy is exact (twice stored: see ``gmm_reference``)
    dy = dv if noise is not None else torch.zeros_like(dv)
    out.update(dsk=dsk, keep=keep, dmu=dmu, dy=dy, dwt=R(ge * pk), quant_mu=quant_mu)
    return out


def _chunks(f, n):
    N = f["y"].numel()
    for i in range(0, N, n):
        yield {k: (None if t is None else t[..., i:i + n]) for k, t in f.items()}


@functools.lru_cache(maxsize=None)
def gmm_reference(name, h16=torch.bfloat16, what="fwd"):
    """{output: {"ref", "unit"[, "store"]}} of a case, fp64, in the kernel's layout.  what = "fwd": y_hat (exact), symbols (exact), lik;
    "bwd": dy, dscales, dmeans (B, HW, [K,] M) and dweights (B, K, M) with its sum bar as the unit."""
    c = GMM[name]
    B, HW, M, K = c["B"], c["H"] * c["W"], c["M"], c["K"]
    f = _flat(c, gmm_operands(name, h16))
    fast = fast_path(c, what)
    acc = {}
    for part in _chunks(f, CHUNK):
        R = Slots()
        o = gmm_chain(c, part, R, fast, what == "bwd")
        if what == "fwd":
            L = o["L"].detach()
            floor = L < LIK_BOUND
            res = dict(lik_ref=torch.where(floor, torch.full_like(L, LIK_BOUND), L), lik_unit=torch.where(floor, torch.zeros_like(L), R.unit(o["L"])),
                       v=o["v"].detach(), L=L)
        else:
            uds = R.unit(o["dsk"])
            dsk, keep = o["dsk"].detach(), o["keep"]
            res = dict(dsc_ref=torch.where(keep, dsk, torch.zeros_like(dsk)),
                       dsc_unit=torch.where(keep | (dsk.abs() <= uds), uds, torch.zeros_like(uds)),
                       dmu_ref=o["dmu"].detach(), dmu_unit=R.unit(o["dmu"]) if o["dmu"].requires_grad else torch.zeros_like(dsk),
                       dy_ref=o["dy"].detach(), dy_unit=R.unit(o["dy"]) if o["dy"].requires_grad else torch.zeros_like(o["dy"]),
                       dwt=o["dwt"].detach(), dwt_unit=R.unit(o["dwt"]), L=o["L"].detach())
        for k, t in res.items():
            acc.setdefault(k, []).append(t)
    acc = {k: torch.cat(t, -1) for k, t in acc.items()}
    lat = lambda t: t.reshape(B, HW, M)
    comp = lambda t: t.reshape(K, B, HW, M).permute(1, 2, 0, 3).contiguous()
    if what == "fwd":
        ydt = {None: _sdt(c, h16), "h16": h16, "f32": torch.float32}[c["f32in"]]
        v = lat(acc["v"])
        assert torch.equal(v.to(ydt).double(), v), "y_hat must be exact in its storage type"
        mu0 = gmm_operands(name, h16)["means"][:, :, 0]
        sym = v - mu0 if (c["umq"] and c["mode"] == "round") else v
        return dict(y_hat=v, symbols=sym, lik=dict(ref=lat(acc["lik_ref"]), unit=lat(acc["lik_unit"])), L=lat(acc["L"]))
    sdt = _sdt(c, h16)
    out = dict(L=lat(acc["L"]))
    for key, r, u, shape in (("dy", "dy_ref", "dy_unit", lat), ("dscales", "dsc_ref", "dsc_unit", comp), ("dmeans", "dmu_ref", "dmu_unit", comp)):
        ref = shape(acc[r])
        twice = 2.0 if (key == "dmeans" and c["umq"] and c["mode"] == "round" and c["gy"]) else 1.0     # stored, reloaded, stored again
        unit = shape(acc[u])
        out[key] = dict(ref=ref, unit=unit, store=storage(ref, sdt, twice) * ((ref != 0) | (unit > 0)))
    if c["weights"]:
        t, tu = comp(acc["dwt"]), comp(acc["dwt_unit"])             # (B, HW, K, M)
        out["dweights"] = dict(ref=t.sum(1), unit=C_BAR * math.sqrt(HW) * U24 * t.abs().sum(1) + tu.sum(1))
        out["dwt_terms"] = t
    return out


def gmm_evaluate(name, h16=torch.bfloat16, what="fwd", dtype=torch.float64, fast=None, mut=(), ops=None, emulate=None):
    """The chain without slots in ``dtype`` (torch's own fp32 evaluation, or a mutated fp64 result), shaped like ``gmm_reference``'s refs."""
    c = GMM[name]
    B, HW, M, K = c["B"], c["H"] * c["W"], c["M"], c["K"]
    f = _flat(c, ops if ops is not None else gmm_operands(name, h16))
    with torch.no_grad():
        o = gmm_chain(c, f, NoSlots(), fast_path(c, what) if fast is None else fast, what == "bwd", dtype=dtype, mut=mut, emulate=emulate)
    lat = lambda t: t.double().reshape(B, HW, M)
    comp = lambda t: t.double().reshape(K, B, HW, M).permute(1, 2, 0, 3).contiguous()
    if what == "fwd":
        return dict(y_hat=lat(o["v"]), lik=lat(torch.maximum(o["L"], torch.tensor(LIK_BOUND, dtype=dtype))))
    out = dict(dy=lat(o["dy"]), dscales=comp(torch.where(o["keep"], o["dsk"], torch.zeros_like(o["dsk"]))), dmeans=comp(o["dmu"]))
    if c["weights"]:
        out["dwt_terms"] = comp(o["dwt"])
        out["dweights"] = comp(o["dwt"]).sum(1)
    return out


# ====================================================================================================== EntropyBottleneck: cases
# The [C][64] parameter table (layout in csrc/entropy.hip): [0, 33) matrices (3x1, 3x3, 3x3, 3x3, 1x3, row-major), [33, 46) biases, [46, 58)
# factors, 58 the median, 59 "prepared" flag, 60 the likelihood bound.  z / noise / g_zhat: (P, C), the kernel's NHWC order, P = B H W.
# st / mode as above; prepared: the forward reads a hesic_eb_prepare_params table; f32in: fp32 z with z_hat stored as "h16" | "f32"; gz: a
# gradient arrives on z_hat; bwd: the case also runs hesic_eb_backward.
EB_STRIDE, EB_MED, EB_READY, EB_BOUND = 64, 58, 59, 60


def _e(C, B, H, W, st, mode="round", prepared=False, f32in=None, gz=False, bwd=False):
    return dict(C=C, B=B, H=H, W=W, st=st, mode=mode, prepared=prepared, f32in=f32in, gz=gz, bwd=bwd)


EB = {
    "c8_p1_f32": _e(8, 1, 1, 1, "f32", bwd=True),
    "c20_p1_h16_noise": _e(20, 1, 1, 1, "h16", mode="noise", gz=True, bwd=True),
    "c16_p17_f32_noise": _e(16, 1, 1, 17, "f32", mode="noise", gz=True),
    "c20_p17_h16": _e(20, 1, 17, 1, "h16", gz=True, bwd=True),
    "c128_p17_f32_noise": _e(128, 1, 1, 17, "f32", mode="noise", gz=True, bwd=True),
    "c128_p17_h16": _e(128, 1, 17, 1, "h16", bwd=True),
    "c8_p513_h16_noise": _e(8, 1, 27, 19, "h16", mode="noise", bwd=True),
    "c8_p513_f32": _e(8, 1, 19, 27, "f32", gz=True, bwd=True),
    "c20_p4097_f32": _e(20, 1, 17, 241, "f32"),
    "c16_p4097_h16_prepared": _e(16, 1, 241, 17, "h16", prepared=True),
    "c20_p17_prepared_f32": _e(20, 1, 1, 17, "f32", prepared=True),
    "c8_p4097_f32in_h16": _e(8, 1, 17, 241, "f32", prepared=True, f32in="h16"),
    "c20_p17_f32in_f32": _e(20, 1, 17, 1, "f32", prepared=True, f32in="f32"),
}
EB_AUX = {"aux_c8": 8, "aux_c128": 128, "aux_c20": 20}


def eb_params(C, seed):
    """compressai's EntropyBottleneck initialisation (filters (3, 3, 3, 3), init_scale 10) plus noise, fp32-exact: lists of matrices
    (C, rows, cols), biases (C, rows, 1), factors (C, rows, 1) and quantiles (C, 1, 3).  Channels 1 and 2 carry factors near +-3 (tanh
    saturates), the last channel a matrix entry above 20 (softplus's linear branch); medians lie on the 1/16 grid."""
    gen = torch.Generator().manual_seed(seed)
    filt = (1, 3, 3, 3, 3, 1)
    scale = 10.0 ** (1 / 5)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    ms, bs, fs = [], [], []
    for i in range(5):
        init = math.log(math.expm1(1 / scale / filt[i + 1]))
        ms.append(init + 0.3 * rn(C, filt[i + 1], filt[i]))
        bs.append(torch.rand((C, filt[i + 1], 1), generator=gen, dtype=torch.float64) - 0.5)
        if i < 4:
            fs.append(0.5 * rn(C, filt[i + 1], 1))
    fs[0][1 % C, :, 0] = torch.tensor([3.0, -2.9, 3.1], dtype=torch.float64)
    fs[2][2 % C, :, 0] = torch.tensor([-3.0, 2.95, -3.2], dtype=torch.float64)
    ms[1][C - 1, 1, 2] = 20.5
    q = torch.zeros((C, 1, 3), dtype=torch.float64)
    q[:, 0, 1] = _grid(gen, (C,), -2, 2)
    q[:, 0, 0] = q[:, 0, 1] - 10 + rn(C)
    q[:, 0, 2] = q[:, 0, 1] + 10 + rn(C)
    f32 = lambda ts: [t.to(torch.float32).double() for t in ts]
    return f32(ms), f32(bs), f32(fs), q.to(torch.float32).double()


def eb_table(ms, bs, fs, q, lik_bound=LIK_BOUND):
    """The raw table, restated from the layout (fp64 holding fp32 values)."""
    C = q.shape[0]
    t = torch.zeros((C, EB_STRIDE), dtype=torch.float64)
    cols = torch.cat([m.reshape(C, -1) for m in ms] + [b.reshape(C, -1) for b in bs] + [f.reshape(C, -1) for f in fs] + [q[:, 0, 1:2]], 1)
    assert cols.shape[1] == 59
    t[:, :59] = cols
    t[:, EB_BOUND] = lik_bound
    return t


@functools.lru_cache(maxsize=None)
def eb_operands(name, h16=torch.bfloat16):
    c = EB[name]
    C, P = c["C"], c["B"] * c["H"] * c["W"]
    gen = torch.Generator().manual_seed(5000 + sorted(EB).index(name))
    ms, bs, fs, q = eb_params(C, 7000 + C)
    table = eb_table(ms, bs, fs, q)
    med = table[:, EB_MED][None]
    z = med + _grid(gen, (P, C), -12, 12)
    # every ninth element far in a tail, below the likelihood floor: whole numbers (exact in every storage type at this size), both sides
    tail = (torch.arange(P * C) % 9 == 5).reshape(P, C)
    z = torch.where(tail, torch.where(torch.rand((P, C), generator=gen) < 0.5, -1.0, 1.0) * torch.round(_grid(gen, (P, C), 236, 252)), z)
    noise = _grid(gen, (P, C), -0.5, 0.5) if c["mode"] == "noise" else None
    if c["mode"] == "round":
        ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], dtype=torch.float64)
        flat = z.view(-1)
        ti = torch.arange(1, P * C, 7)
        flat[ti] = ties[torch.arange(ti.numel()) % 6] + med.expand(P, C).reshape(-1)[ti]
    g = torch.randn((P, C), generator=gen, dtype=torch.float64).to(torch.float32).double()
    g = torch.where((torch.arange(P * C) % 18 == 5).reshape(P, C), -g.abs(), g)          # every other tail element: g < 0, the mask passes it
    gz = _grid(gen, (P, C), -2, 2) if c["gz"] else None
    o = dict(z=z, noise=noise, g=g, gz=gz, table=table, params=(ms, bs, fs, q))
    for _ in range(8):              # no unclamped likelihood within a factor 2 of the bound: an offender moves onto the median
        with torch.no_grad():
            L = eb_chain(c, o, NoSlots(), False)["L"]
        off = (L > LIK_BOUND / 2) & (L < LIK_BOUND * 2)
        if not bool(off.any()):
            break
        o["z"] = torch.where(off, med.expand(P, C), o["z"])
    sdt = _sdt(c, h16)
    for k in ("z", "noise", "gz"):
        assert o[k] is None or torch.equal(o[k].to(sdt).double(), o[k]), "operands must be exact in the storage type"
    return o


# ====================================================================================================== EntropyBottleneck: chain
def _eb_prepare(table, n, R, dtype, need_sg, mut=()):
    """softplus(matrices), biases, tanh(factors) [, sigmoid(raw matrices)] of every channel, expanded to the element shape (n, C) BEFORE
    their slots: each element gets its own share of a per-channel rounding."""
    C = table.shape[0]
    col = lambda i: table[:, i].to(dtype)[None].expand(n, C)
    sp = []
    for i in range(33):
        x = col(i)
        sp.append(torch.where(x > 20, x, R(torch.log1p(R(torch.exp(x.clamp(max=20.0)), K_EXP)), K_LOG1P)))
    b = [col(33 + i) for i in range(13)]
    tf = [R(torch.tanh(col(46 + i)), K_TANH) for i in range(12)]
    sg = None
    if need_sg:
        sg = [R(1.0 / R(1.0 + R(torch.exp(-col(i)), K_EXP))) for i in range(33)]
        if "no_sigmoid_layer1" in mut:
            for i in range(3, 12):
                sg[i] = torch.ones_like(sg[i])
    return sp, b, tf, sg


def _dot3(R, m, h, b):
    return R(R(R(R(m[0] * h[0]) + R(m[1] * h[1])) + R(m[2] * h[2])) + b)


def _eb_logits(q, v, R):
    """eb_logits: (out, pre-activation tanh's, layer inputs)."""
    sp, b, tf, _ = q
    t = [R(R(sp[r] * v) + b[r]) for r in range(3)]
    ths, hin = [], [None]
    for l in range(4):
        if l:
            hin.append(h)
            t = [_dot3(R, sp[3 + (l - 1) * 9 + r * 3:3 + (l - 1) * 9 + r * 3 + 3], h, b[3 * l + r]) for r in range(3)]
        th = [R(torch.tanh(x), K_TANH) for x in t]
        ths.append(th)
        h = [R(t[r] + R(tf[3 * l + r] * th[r])) for r in range(3)]
    hin.append(h)
    return _dot3(R, sp[30:33], h, b[12]), ths, hin


def _eb_logits_bwd(q, v, gout, R):
    """eb_logits_bwd: (dv, {column: term}) of one logits evaluation, as the formulas the kernel evaluates."""
    sp, b, tf, sg = q
    _, ths, hin = _eb_logits(q, v, R)
    col = {45: gout}
    dh = []
    for j in range(3):
        if sg is not None:
            col[30 + j] = R(R(gout * hin[4][j]) * sg[30 + j])
        dh.append(R(gout * sp[30 + j]))
    for l in (3, 2, 1):
        dpre = []
        for r in range(3):
            th, f = ths[l][r], tf[3 * l + r]
            col[46 + 3 * l + r] = R(R(dh[r] * th) * R(1.0 - R(f * f)))
            dpre.append(R(dh[r] * R(1.0 + R(f * R(1.0 - R(th * th))))))
            col[33 + 3 * l + r] = dpre[r]
        nh = [None] * 3
        for r in range(3):
            for j in range(3):
                k = 3 + (l - 1) * 9 + r * 3 + j
                if sg is not None:
                    col[k] = R(R(dpre[r] * hin[l][j]) * sg[k])
                t = R(sp[k] * dpre[r])
                nh[j] = t if nh[j] is None else R(nh[j] + t)
        dh = nh
    dv = None
    for r in range(3):
        th, f = ths[0][r], tf[r]
        col[46 + r] = R(R(dh[r] * th) * R(1.0 - R(f * f)))
        dpre = R(dh[r] * R(1.0 + R(f * R(1.0 - R(th * th)))))
        col[33 + r] = dpre
        if sg is not None:
            col[r] = R(R(dpre * v) * sg[r])
        t = R(dpre * sp[r])
        dv = t if dv is None else R(dv + t)
    return dv, col


def _sigmoid(R, x):
    return R(1.0 / R(1.0 + R(torch.exp(-x), K_EXP)))


def eb_chain(c, o, R, backward, dtype=torch.float64, mut=()):
    """eb_fwd_kernel / eb_bwd_kernel on (P, C) operands: v, L (unclamped) and, with ``backward``, dz and the 59 column terms
    {column: (2, P, C) upper / lower evaluation} (the median column: (1, P, C))."""
    cv = lambda t: None if t is None else t.to(dtype)
    z, noise, g, gz = cv(o["z"]), cv(o["noise"]), cv(o["g"]), cv(o["gz"])
    P, C = z.shape
    med = o["table"][:, EB_MED].to(dtype)[None].expand(P, C)
    bound = o["table"][:, EB_BOUND].to(dtype)[None].expand(P, C)
    rnd = (lambda t: torch.sign(t) * torch.floor(t.abs() + 0.5)) if "round_away" in mut else torch.round
    v = z + noise if noise is not None else rnd(z - med) + med
    q = _eb_prepare(o["table"], P, R, dtype, backward, mut)
    lo, _, _ = _eb_logits(q, v - 0.5, R)
    up, _, _ = _eb_logits(q, v + 0.5, R)
    s = -torch.sign(R(lo + up)).detach()
    A, Bv = _sigmoid(R, s * up), _sigmoid(R, s * lo)
    dlt = R(A - Bv)
    out = dict(v=v, L=dlt.abs(), bound=bound)
    if not backward:
        return out
    keep = (dlt.detach().abs() >= bound) | (g < 0)
    if "no_lik_mask" in mut:
        keep = torch.ones_like(keep)
    if "no_lik_gneg" in mut:
        keep = dlt.detach().abs() >= bound
    sgg = torch.sign(dlt.detach()) * torch.where(keep, g, torch.zeros_like(g))
    gU = R(R(sgg * A) * R(1.0 - A)) * s
    gL = -R(R(sgg * Bv) * R(1.0 - Bv)) * s
    dvU, cU = _eb_logits_bwd(q, v + 0.5, gU, R)
    dvL, cL = _eb_logits_bwd(q, v - 0.5, gL, R)
    dv = R.add(dvU, dvL)
    if gz is not None:
        dv = R.add(dv, gz)
    cols = {k: torch.stack((cU[k], cL[k])) for k in cU}
    if noise is not None:
        dz = dv
    else:
        dz = torch.zeros_like(dv)
        if "no_median" not in mut:
            cols[EB_MED] = dv[None]
    out.update(dz=dz, cols=cols)
    return out


@functools.lru_cache(maxsize=None)
def eb_reference(name, h16=torch.bfloat16, what="fwd"):
    """fwd: z_hat, symbols (exact), lik {"ref", "unit"}; bwd: dz {"ref", "unit", "store"} and dparams (C, 59) with its sum bar as the unit:
    C_BAR sqrt(n) 2^-24 S + sum of the terms' units, n the number of terms of the column (2 P: an upper and a lower evaluation per pixel)."""
    c = EB[name]
    o = eb_operands(name, h16)
    P, C = o["z"].shape
    R = Slots()
    r = eb_chain(c, o, R, what == "bwd")
    L = r["L"].detach()
    if what == "fwd":
        floor = L < r["bound"]
        ydt = {None: _sdt(c, h16), "h16": h16, "f32": torch.float32}[c["f32in"]]
        v = r["v"].detach()            # exact in fp32; a 16-bit z_hat is its one deterministic rounding
        assert torch.equal(v.to(torch.float32).double(), v)
        med = o["table"][:, EB_MED][None]
        return dict(z_hat=v.to(ydt).double(), symbols=v - med, L=L,
                    lik=dict(ref=torch.where(floor, r["bound"], L), unit=torch.where(floor, torch.zeros_like(L), R.unit(r["L"]))))
    sdt = _sdt(c, h16)
    out = dict(L=L)
    dz = r["dz"]
    unit = R.unit(dz) if dz.requires_grad else torch.zeros_like(dz)
    out["dz"] = dict(ref=dz.detach(), unit=unit, store=storage(dz.detach(), sdt) * ((dz.detach() != 0) | (unit > 0)))
    ref = torch.zeros((C, 59), dtype=torch.float64)
    bar = torch.zeros((C, 59), dtype=torch.float64)
    terms = {}
    for k, t in r["cols"].items():
        n = t.shape[0] * P
        u = R.unit(t.sum(0)) if t.requires_grad else torch.zeros((P, C), dtype=torch.float64)     # upper + lower share their per-channel nodes
        td = t.detach()
        ref[:, k] = td.sum((0, 1))
        bar[:, k] = C_BAR * math.sqrt(n) * U24 * td.abs().sum((0, 1)) + u.sum(0)
        terms[k] = td
    out["dparams"] = dict(ref=ref, unit=bar)
    out["terms"] = terms
    return out


def eb_evaluate(name, h16=torch.bfloat16, what="fwd", dtype=torch.float64, mut=()):
    c = EB[name]
    o = eb_operands(name, h16)
    with torch.no_grad():
        r = eb_chain(c, o, NoSlots(), what == "bwd", dtype=dtype, mut=mut)
    if what == "fwd":
        return dict(z_hat=r["v"].double(), lik=torch.maximum(r["L"], r["bound"]).double())
    C = o["z"].shape[1]
    dp = torch.zeros((C, 59), dtype=torch.float64)
    for k, t in r["cols"].items():
        dp[:, k] = t.double().sum((0, 1))
    return dict(dz=r["dz"].double(), dparams=dp, terms={k: t.double() for k, t in r["cols"].items()})


# ------------------------------------------------------------------------------------------------------------------- aux loss
def tail_target(tail_mass=1e-9):
    """logf(2.f / tail_mass - 1.f) as the host computes it in fp32."""
    tm = torch.tensor(tail_mass, dtype=torch.float32)
    return float(torch.log(torch.tensor(2.0, dtype=torch.float32) / tm - 1.0))


@functools.lru_cache(maxsize=None)
def aux_reference(name, accumulate=False):
    """EntropyBottleneck.loss and its quantile gradient: loss {"ref", "unit"} (scalar, sum bar over the 3 C terms) and dquantiles (C, 3).
    The target is the host's fp32 logf: one slot of 2 ulps (the division and the logarithm)."""
    C = EB_AUX[name]
    ms, bs, fs, q = eb_params(C, 7000 + C)
    table = eb_table(ms, bs, fs, q, 0.0)
    R = Slots()
    prm = _eb_prepare(table, 3, R, torch.float64, False)
    v = q[:, 0, :].t().contiguous()                               # (3, C)
    t_hi = math.log(2.0 / 1e-9 - 1.0)
    tgt = R(torch.tensor([-t_hi, 0.0, t_hi], dtype=torch.float64)[:, None].expand(3, C), 2.0)
    logits, _, _ = _eb_logits(prm, v, R)
    diff = R(logits - tgt)
    assert float(diff.detach().abs().min()) > 1e-3, "the sign of every difference must be the reference's to decide"
    part = diff.abs()
    dq, _ = _eb_logits_bwd(prm, v, torch.sign(diff.detach()), R)
    old = None
    if accumulate:
        old = _grid(torch.Generator().manual_seed(C), (3, C), -2, 2)
        dq = R(old + dq)
    pd = part.detach()
    loss_bar = C_BAR * math.sqrt(3 * C) * U24 * float(pd.sum()) + float(R.unit(part).sum())
    return dict(params=(ms, bs, fs, q), table=table, old=None if old is None else old.t().contiguous(),
                loss=dict(ref=pd.sum().reshape(1), unit=torch.tensor([loss_bar], dtype=torch.float64)),
                dq=dict(ref=dq.detach().t().contiguous(), unit=R.unit(dq).t().contiguous()), terms=pd)


@functools.lru_cache(maxsize=None)
def prepare_reference(C):
    """hesic_eb_prepare_params, per slot: softplus / tanh to their ulp counts, every other slot exact, slot 59 = 1, slots 61.. = 0."""
    ms, bs, fs, q = eb_params(C, 7000 + C)
    table = eb_table(ms, bs, fs, q)
    R = Slots()
    sp, b, tf, _ = _eb_prepare(table, 1, R, torch.float64, False)
    ref = table.clone()
    unit = torch.zeros_like(ref)
    for i in range(33):
        ref[:, i] = sp[i].detach()[0]
        unit[:, i] = R.unit(sp[i])[0] if sp[i].requires_grad else 0.0
    for i in range(12):
        ref[:, 46 + i] = tf[i].detach()[0]
        unit[:, 46 + i] = R.unit(tf[i])[0]
    ref[:, EB_READY] = 1.0
    return dict(raw=table, ref=ref, unit=unit)
