"""fp64 reference with a per-element error model for the GDN / IGDN kernels, forward and backward (a plain module, not a conftest).

    beta' = max(beta, sqrt(beta_min + 2^-36))^2 - 2^-36,  gamma' = max(gamma, 2^-18)^2 - 2^-36
    n[p,i] = beta'[i] + sum_j gamma'[i,j] sq[p,j],  sq = x^2;   y = x n^-1/2 (GDN) | x n^1/2 (IGDN)
    dn = -1/2 g x n^-3/2 | +1/2 g x n^-1/2;   dx[p,j] = g r + 2 x sum_i gamma'[i,j] dn[p,i]
    dgamma'[i,j] = sum_p dn[p,i] sq[p,j],  dbeta'[i] = sum_p dn[p,i]
    dtheta = dtheta' * 2 max(theta, bound), passed where theta >= bound or dtheta < 0 (LowerBound), else exactly 0

``reference()`` evaluates this closed form in fp64 on (P, C) operands that are exactly what the kernels receive (x and gy hold values
representable in the storage type, the parameters are fp32); ``reference_autograd()`` is the oracle's autograd in fp64, and
tests/test_gdn_ref_cpu.py holds one against the other.  ``bars()`` gives every element of y, dx, dgamma, dbeta a UNIT bar; a test accepts
|got - ref| <= C_BAR * unit (+ a storage term where noted).  Both regimes are statistical: the root of a sum of squared per-term bounds.

fp32 storage (any C; also the arithmetic of the 3-channel 16-bit kernels, which compute in fp32 and round on store):
    e_n = sqrt(C + 1) 2^-24 S_n,  S_n = sum of the |terms| of n (each gamma' + 2^-36: the reparametrisation's own rounding is relative to
    t^2, not to t^2 - 2^-36),  rho = e_n / n;  elementwise chains add their rounding count linearly (3 for y, 6 for dn): a handful of
    roundings is no statistic.  dn carries k rho (k = 3/2 | 1/2); dx, dgamma', dbeta' propagate e_dn by root-sum-square and add
    sqrt(terms) 2^-24 S for their own fp32 sums (any order: block partials, atomics, MFMA accumulation).
    3-channel 16-bit kernels: bar = C_BAR * unit + u |ref| on y and dx.

16-bit storage, C = 128 (gdn128_kernel<h16_t>, gdn128_bwd_kernel), u = 2^-8 (bf16) | 2^-11 (f16).  These kernels round BY DESIGN and the
model, not the reference, accounts for each rounding: gamma' and x^2 go to 16 bit (the f16 forward scales x^2 by 2^-6 and gamma' by 2^6,
exact powers of two), dn goes to 16 bit before the second and third GEMM, y and dx go to 16 bit on store:
    dn_i^2   = sum_j (u gamma'_ij + h_g)^2 sq_j^2 + gamma'_ij^2 (u sq_j + h_s)^2            rho_i = dn_i / n_i
    bar_y    = u |y| + h + 1/2 rho |y|
    ddn_i    = |dn_i| sqrt(u^2 + (k rho_i)^2) + h
    bar_dx_j = u |dx_j| + h + sqrt((1/2 rho_j |g_j r_j|)^2 + (2 x_j)^2 (sum_i gamma'_ij^2 ddn_i^2 + sum_i (u gamma'_ij + h_g)^2 dn_i^2))
    bar_dgamma'_ij = sqrt(sum_p ddn_pi^2 sq_pj^2 + sum_p dn_pi^2 (u sq_pj + h_s)^2),   bar_dbeta'_i = sqrt(sum_p ddn_pi^2)
plus the fp32 unit of the first regime.  The h terms are binary16's gradual underflow (half of the smallest subnormal, 2^-25; x^2 scaled by
2^-6 in the forward: 2^-19 after unscaling); they are 0 for bf16, whose range is fp32's.  They matter for a single pixel only: |dn| < 6e-5
is a subnormal half, and with P = 1 nothing else sits in that sum.

Raw-parameter bars are the primed ones times the chain factor 2 max(theta, bound) (+ 2 roundings).  A clamped parameter (theta < bound)
has the masked reference as its expected value -- exactly 0 where the fp64 dtheta' >= 0 -- and its own bar: a sign that flips within noise
is accepted and nothing else is.  No element is left out of a comparison.

C_BAR = 8.  tests/test_gdn_ref_cpu.py measures an fp64 evaluation that applies exactly the by-design roundings (``emulate``) against the
unit bars: the worst ratio over all cases must stay below C_BAR / 2, since a kernel adds only the 1-ulp v_rsq_f32 / v_sqrt_f32
approximations and fp32 ordering on top.  Measured values: profiles/gdn_parity.json.
"""
import functools
import math

import torch

from hesic_amd import synthetic

C_BAR = 8.0
U24 = 2.0 ** -24
PED = 2.0 ** -36
GAMMA_BOUND = 2.0 ** -18
TILE = 128                     # pixels per tile of the 16-bit C = 128 kernels
MAX_BLOCKS = 256               # gdn128_bwd_kernel's launch cap: one parameter-gradient partial per block

FMT = {
    "f32": {"dtype": torch.float32, "u": 0.0, "h": 0.0, "h_s": 0.0, "h_g": 0.0},
    "bf16": {"dtype": torch.bfloat16, "u": 2.0 ** -8, "h": 0.0, "h_s": 0.0, "h_g": 0.0},
    "f16": {"dtype": torch.float16, "u": 2.0 ** -11, "h": 2.0 ** -25, "h_s": 2.0 ** -19, "h_g": 2.0 ** -25},
}


def beta_bound(beta_min=1e-6):
    """sqrtf(beta_min + 2^-36) as the host code forms it: fp32 sum, fp32 root."""
    return float(torch.sqrt(torch.tensor(beta_min, dtype=torch.float32) + torch.tensor(PED, dtype=torch.float32)))


def rnd(t, fmt):
    """``t`` (fp64) rounded to the storage type, back in fp64."""
    return t if fmt == "f32" else t.to(FMT[fmt]["dtype"]).double()


def _chain(theta, dprime, bound, mask="rule"):
    """(masked raw gradient, unmasked raw gradient, chain factor) of one parameter tensor."""
    f = 2.0 * theta.clamp_min(bound)
    g = dprime * f
    clamped = theta < bound
    if mask == "rule":
        keep = ~clamped | (g < 0)
    elif mask == "ignored":
        keep = torch.ones_like(clamped)
    else:                                            # "inverted": the rule's complement on the clamped entries
        keep = ~clamped | ~(g < 0)
    return torch.where(keep, g, torch.zeros((), dtype=g.dtype)), g, f


def reference(x, gy, beta_raw, gamma_raw, inverse, beta_min=1e-6):
    """x, gy (P, C) (gy None: forward only), beta_raw (C,), gamma_raw (C, C).  Everything returned is fp64."""
    x = x.double()
    P, C = x.shape
    bb = beta_bound(beta_min)
    th_b, th_g = beta_raw.double(), gamma_raw.double()
    bp = th_b.clamp_min(bb) ** 2 - PED
    gp = th_g.clamp_min(GAMMA_BOUND) ** 2 - PED
    sq = x * x
    n = bp + sq @ gp.T
    r = n.sqrt() if inverse else n.rsqrt()
    R = {"C": C, "P": P, "inverse": bool(inverse), "k": 0.5 if inverse else 1.5, "x": x, "sq": sq, "n": n, "r": r, "bp": bp, "gp": gp,
         "beta_bound": bb, "theta_b": th_b, "theta_g": th_g, "S_n": (bp + PED) + sq @ (gp + PED).T, "ref": {"y": x * r}}
    if gy is None:
        return R
    g = gy.double()
    dn = 0.5 * g * x / n.sqrt() if inverse else -0.5 * g * x * n ** -1.5
    t1 = g * r
    s = dn @ gp                                      # s[p, j] = sum_i gamma'[i, j] dn[p, i]
    dgp, dbp = dn.T @ sq, dn.sum(0)
    dgamma, dg_raw, fg = _chain(th_g, dgp, GAMMA_BOUND)
    dbeta, db_raw, fb = _chain(th_b, dbp, bb)
    R.update(g=g, dn=dn, t1=t1, s=s, dgp=dgp, dbp=dbp, fg=fg, fb=fb, dg_raw=dg_raw, db_raw=db_raw)
    R["ref"].update(dx=t1 + 2.0 * x * s, dgamma=dgamma, dbeta=dbeta)
    return R


def reference_autograd(x, gy, beta_raw, gamma_raw, inverse, beta_min=1e-6):
    """y, dx, dgamma, dbeta by autograd of the oracle's gdn in fp64 (LowerBound rule included)."""
    from oracle import hesic_oracle as O
    P, C = x.shape
    x4 = x.double().T.reshape(1, C, P, 1).clone().requires_grad_()
    b, g = beta_raw.double().clone().requires_grad_(), gamma_raw.double().clone().requires_grad_()
    y = O.gdn(x4, b, g, inverse, beta_min)
    y.backward(gy.double().T.reshape(1, C, P, 1))
    back = lambda t: t.detach().reshape(C, P).T
    return {"y": back(y), "dx": back(x4.grad), "dgamma": g.grad, "dbeta": b.grad}


# ------------------------------------------------------------------------------------------------------------------------ the error model
def _unit32(R):
    C, P, k = R["C"], R["P"], R["k"]
    x, sq, gp = R["x"], R["sq"], R["gp"]
    rho = math.sqrt(C + 1) * U24 * R["S_n"] / R["n"]
    out = {"y": R["ref"]["y"].abs() * (0.5 * rho + 3 * U24)}
    if "dn" not in R:
        return out
    dn = R["dn"]
    e_dn = dn.abs() * (k * rho + 6 * U24)
    e_s = ((e_dn ** 2) @ (gp ** 2)).sqrt() + math.sqrt(C) * U24 * (dn.abs() @ (gp + PED))
    out["dx"] = R["t1"].abs() * (0.5 * rho + 3 * U24) + 2 * x.abs() * e_s + 3 * U24 * (2 * x * R["s"]).abs() + U24 * R["ref"]["dx"].abs()
    out["dgp"] = ((e_dn ** 2).T @ (sq ** 2)).sqrt() + (math.sqrt(P) + 2) * U24 * (dn.abs().T @ sq)
    out["dbp"] = (e_dn ** 2).sum(0).sqrt() + math.sqrt(P) * U24 * dn.abs().sum(0)
    return out


def _unit16(R, fmt):
    f = FMT[fmt]
    u, h, h_s, h_g, k = f["u"], f["h"], f["h_s"], f["h_g"], R["k"]
    x, sq, gp, n = R["x"], R["sq"], R["gp"], R["n"]
    ug2, us2 = (u * gp + h_g) ** 2, (u * sq + h_s) ** 2
    rho = ((sq ** 2) @ ug2.T + us2 @ (gp ** 2).T).sqrt() / n
    y = R["ref"]["y"].abs()
    out = {"y": u * y + h + 0.5 * rho * y}
    if "dn" not in R:
        return out
    dn = R["dn"]
    d_dn = dn.abs() * (u * u + (k * rho) ** 2).sqrt() + h
    out["dx"] = u * R["ref"]["dx"].abs() + h + ((0.5 * rho * R["t1"].abs()) ** 2 + (2 * x) ** 2 * ((d_dn ** 2) @ (gp ** 2) + (dn ** 2) @ ug2)).sqrt()
    out["dgp"] = ((d_dn ** 2).T @ (sq ** 2) + (dn ** 2).T @ us2).sqrt()
    out["dbp"] = (d_dn ** 2).sum(0).sqrt()
    return out


def bars(R, fmt):
    """{output: (unit, extra)}: a test accepts |got - ref| <= c * unit + extra.  ``extra`` is the 16-bit storage term of the kernels that
    compute in fp32 (C != 128) and 0 otherwise."""
    un = _unit32(R)
    extra = {q: torch.zeros_like(v) for q, v in un.items()}
    if fmt != "f32":
        if R["C"] == 128:
            for q, v in _unit16(R, fmt).items():
                un[q] = un[q] + v
        else:
            for q in ("y", "dx"):
                if q in un:
                    extra[q] = FMT[fmt]["u"] * R["ref"][q].abs()
    out = {"y": (un["y"], extra["y"])}
    if "dn" in R:
        out["dx"] = (un["dx"], extra["dx"])
        out["dgamma"] = (un["dgp"] * R["fg"] + 2 * U24 * R["dg_raw"].abs(), torch.zeros_like(un["dgp"]))
        out["dbeta"] = (un["dbp"] * R["fb"] + 2 * U24 * R["db_raw"].abs(), torch.zeros_like(un["dbp"]))
    return out


def check(ref, bar, got, q, c=C_BAR, extra=None):
    """(ok, ratio, message) of one output: every element of ``got`` within c * unit + extra of ``ref``.  ratio = max_e (|err_e| - extra_e)+ /
    unit_e; an element whose unit is 0 must be exact.  ``extra`` adds to the bar's own extra term (an accumulating call's 2^-24 |sum|)."""
    unit, ex = bar
    if extra is not None:
        ex = ex + extra
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    over = (err - ex).clamp_min(0)
    live = unit > 0
    ratio_e = torch.where(live, over / unit.clamp_min(1e-300), torch.where(over > 0, torch.full_like(over, float("inf")), torch.zeros_like(over)))
    ratio_e = torch.where(torch.isnan(got), torch.full_like(ratio_e, float("inf")), ratio_e)
    ratio = float(ratio_e.max())
    bad = ~(ratio_e <= c)
    msg = ""
    if bool(bad.any()):
        w = int(torch.argmax(ratio_e))
        if ref.dim() == 2 and q in ("y", "dx"):
            p, ch = divmod(w, ref.shape[1])
            where = f"pixel {p} channel {ch} tile {p // TILE}"
        elif ref.dim() == 2:
            i, j = divmod(w, ref.shape[1])
            where = f"row {i} column {j}"
        else:
            where = f"channel {w}"
        msg = (f"{q}: {int(bad.sum())} of {bad.numel()} elements outside {c:g} x their bar; worst ratio {ratio:.4g} at {where}: "
               f"got {float(got.reshape(-1)[w]):.9g} ref {float(ref.reshape(-1)[w]):.9g} unit bar {float(unit.reshape(-1)[w]):.3g}")
    return not bool(bad.any()), ratio, msg


def outside(ref, bar, got, c=C_BAR):
    """bool tensor: the elements of ``got`` outside c * unit + extra."""
    unit, ex = bar
    return ~((got.double().reshape(ref.shape) - ref).abs() <= c * unit + ex)


# --------------------------------------------------------------------------------------------------------------- the by-design roundings
MUTATIONS = ("drop_last_pixel", "drop_tile", "drop_partial", "mask_inverted", "mask_ignored", "gamma_untransposed", "gdn_dn_for_igdn")


def dropped_pixels(R, mut):
    """How many pixels a dropping mutation takes out of the parameter sums."""
    P = R["P"]
    ntiles = (P + TILE - 1) // TILE
    nb = min(ntiles, MAX_BLOCKS)
    if mut == "drop_last_pixel":
        return 1
    if mut == "drop_tile":
        return min(P, TILE)
    return int(((torch.arange(P) // TILE) % nb == nb - 1).sum())


def mutations_of(R, fmt):
    """The mutations a case has.  A block partial exists beyond the first tile, the wrong dn formula in an IGDN case only.  m dropped terms
    of P (random signs, rms size t) change a sum by sqrt(m) t; the bar of that sum is C_BAR u sqrt(2 P) t in the 16-bit C = 128 kernels and
    C_BAR sqrt(P) 2^-24 P t in fp32 arithmetic, so the drop is above the bar only while  m > 2 P (C_BAR u)^2  |  m > (C_BAR P^1.5 2^-24)^2:
    one pixel up to P = 512 (bf16), 32,768 (f16), 16,384 (fp32).  Beyond that no per-element test can see it, and the case does not have it:
    the finish cases from nb = 16 on (bf16) and the 32,769-pixel backward cannot see ONE lost row in dgamma or dbeta -- there that row shows
    in its own dx, and the loss of a tile or a block partial in the parameter sums."""
    out = ["mask_inverted", "mask_ignored", "gamma_untransposed"]
    P = R["P"]
    u = FMT[fmt]["u"] if R["C"] == 128 else 0.0
    floor = 2 * P * (C_BAR * u) ** 2 if u else (C_BAR * P ** 1.5 * U24) ** 2
    for mut in ("drop_last_pixel", "drop_tile") + (("drop_partial",) if P > TILE else ()):
        if dropped_pixels(R, mut) > floor:
            out.append(mut)
    if R["inverse"]:
        out.append("gdn_dn_for_igdn")
    return out


def emulate(R, fmt, mut=None):
    """y, dx, dgamma, dbeta evaluated in fp64 with exactly the roundings the kernels of (C, fmt) make by design -- for the 16-bit C = 128
    kernels the list in the module docstring, for other 16-bit kernels the store of y and dx, for fp32 none -- and, with ``mut``, one
    deliberate defect (tests/test_gdn_ref_cpu.py)."""
    C, P, inverse = R["C"], R["P"], R["inverse"]
    x, sq, gp, bp, g = R["x"], R["sq"], R["gp"], R["bp"], R["g"]
    wide16 = fmt != "f32" and C == 128
    r16 = (lambda t: rnd(t, fmt)) if wide16 else (lambda t: t)
    gp16, sq16 = r16(gp), r16(sq)
    if wide16 and fmt == "f16":                      # the forward's range scaling: x^2 2^-6, gamma' 2^6
        n_f = bp + (r16(sq / 64.0) * 64.0) @ (r16(gp * 64.0) / 64.0).T
    else:
        n_f = bp + sq16 @ gp16.T
    y = rnd(x * (n_f.sqrt() if inverse else n_f.rsqrt()), fmt)
    n = bp + sq16 @ gp16.T
    r = n.sqrt() if inverse else n.rsqrt()
    if inverse and mut != "gdn_dn_for_igdn":
        dn = 0.5 * g * x / n.sqrt()
    else:
        dn = -0.5 * g * x * n ** -1.5
    dn = r16(dn)
    s = dn @ (gp16.T if mut == "gamma_untransposed" else gp16)
    dx = rnd(g * r + 2.0 * x * s, fmt)
    # parameter sums: tile t goes to block t % nb, the finish adds the nb block partials
    ntiles = (P + TILE - 1) // TILE
    nb = min(ntiles, MAX_BLOCKS)
    dnp = dn.clone()
    if mut == "drop_last_pixel":
        dnp[P - 1] = 0
    elif mut == "drop_tile":
        dnp[:TILE] = 0
    elif mut == "drop_partial":
        tiles = torch.arange(P) // TILE
        dnp[tiles % nb == nb - 1] = 0
    dgp, dbp = dnp.T @ sq16, dnp.sum(0)
    mask = {"mask_inverted": "inverted", "mask_ignored": "ignored"}.get(mut, "rule")
    return {"y": y, "dx": dx, "dgamma": _chain(R["theta_g"], dgp, GAMMA_BOUND, mask)[0], "dbeta": _chain(R["theta_b"], dbp, R["beta_bound"], mask)[0]}


# ------------------------------------------------------------------------------------------------------------------------ the case table
def _cases():
    """tag -> {C, P, fmt, inverse, layout ("nhwc" | "planar": B images of P / B pixels), bwd (False: forward only), group}."""
    T = {}

    def add(group, C, P, fmt, bwd=True, layout="nhwc", B=1):
        for inv in (False, True):
            tag = f"{group}_c{C}_{'planar' + str(B) + 'x' if layout == 'planar' else 'p'}{P // B}_{fmt}_{'igdn' if inv else 'gdn'}"
            T[tag] = {"C": C, "P": P, "B": B, "fmt": fmt, "inverse": inv, "layout": layout, "bwd": bwd, "group": group}
    for fmt in ("bf16", "f16"):
        for P in (1, 129, 256):                      # one row; a second tile of one row; exact tiles
            add("wide16", 128, P, fmt)
        add("stride16", 128, 256 * 128 + 1, fmt)     # backward: block 0 takes tiles 0 and 256, the latter with one row
        add("stride16", 128, 512 * 128 + 1, fmt, bwd=False)          # the forward's cap of 512 blocks
    for nb in (1, 16, 17, 33):                       # the finish kernels' two-accumulator loop: nb <= 16, 17 .. 32, > 32
        add("finish", 128, 128 * nb, "bf16")
    for nb in (17, 33):                              # the float16 library compiles its own finish kernels: both accumulators, and the tail
        add("finish", 128, 128 * nb, "f16")
    for P in (1, 65, 129):                           # gdn128_kernel<float> (64-pixel tiles), three-pass backward
        add("wide32", 128, P, "f32")
    add("wide32", 128, 256 * 64 + 1, "f32", bwd=False)               # forward grid stride (the generic backward is O(P C^2) per launch)
    for fmt in ("f32", "bf16"):
        for P in (1, 513):                           # 513: two blocks of 256 threads, pixel 512 is thread 0 of block 0 on its second trip
            add("small", 3, P, fmt)
        add("small", 3, 2 * 513, fmt, layout="planar", B=2)          # blockIdx.y
        add("small", 3, 1024 * 512 + 1, fmt)         # past the backward's 1024 blocks x 512 and the forward's 2048 x 256 pixels per launch
    for C in (8, 5):
        for P in (1, 2049):                          # gdn_bwd_param_kernel: rows_per_block = 2, a last block of one row
            add("generic", C, P, "f32")
    return T


CASES = _cases()
STRIDE = [t for t, c in CASES.items() if c["P"] * c["C"] >= 2 ** 22]    # the wide grid-stride shapes: their fp64 reference is not cheap


def params(C, salt=0):
    """beta (C,), gamma (C, C) in the reparametrised domain: synthetic's fill, then every 7th gamma pushed to 1e-7, every 11th to a negative
    value, every 13th set to exactly 2^-18 (not clamped: theta >= bound), beta[1] below its bound and beta[2] exactly at it."""
    sd = {"g.beta": torch.zeros(C), "g.gamma": torch.zeros(C, C)}
    synthetic.fill_state_dict_(sd, salt=salt)
    flat = sd["g.gamma"].view(-1)
    flat[::7] = 1e-7
    flat[::11] = -0.05
    flat[::13] = GAMMA_BOUND
    bb = beta_bound()
    sd["g.beta"][1] = 0.5 * bb
    sd["g.beta"][2] = bb
    return sd["g.beta"], sd["g.gamma"]


def _both_signs(R):
    """Both signs of dtheta' occur among the clamped entries (gamma and beta together)."""
    d = torch.cat([R["dgp"][R["theta_g"] < GAMMA_BOUND], R["dbp"][R["theta_b"] < R["beta_bound"]]])
    return bool((d > 0).any()) and bool((d < 0).any())


def make_case(tag):
    """(operands, reference) of a case.  x in +-3, gy in +-1, rounded to the storage type, pixel major (P, C); for a planar case pixel
    p = b * HW + q.  The seed is the first salt at which the reference has both signs of dtheta' among its clamped parameters."""
    c = CASES[tag]
    for salt in range(32):
        name = f"gdnp.{tag}.{salt}."
        dt = FMT[c["fmt"]]["dtype"]
        x = synthetic._uniform(name + "x", (c["P"], c["C"]), -3, 3).to(dt).float()
        gy = synthetic._uniform(name + "g", (c["P"], c["C"]), -1, 1).to(dt).float() if c["bwd"] else None
        beta, gamma = params(c["C"], salt)
        R = reference(x, gy, beta, gamma, c["inverse"])
        if not c["bwd"] or _both_signs(R):
            return {"x": x, "gy": gy, "beta": beta, "gamma": gamma, "salt": salt}, R
    raise AssertionError(f"{tag}: no seed gives both signs of dtheta' among the clamped parameters")


@functools.lru_cache(maxsize=8)
def _cached_case(tag):
    return make_case(tag)


def case(tag):
    """``make_case`` shared and left unchanged.  The cache is bounded (a case holds ~20 fp64 tensors of its shape; the test files also clear it
    when they are done) and the wide grid-stride shapes (0.5 GB of fp64 each) are built per use."""
    return make_case(tag) if tag in STRIDE else _cached_case(tag)


def clear_cache():
    _cached_case.cache_clear()
