#!/usr/bin/env python3
"""bench.py -- stereo-pairs/sec of HESIC encode+decode at 512x512 on N MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of synthetic stereo pairs already resident in HBM:
eval-mode ``HSIC.forward`` (3 analysis passes, hyper path, quantise + likelihood, 2 synthesis passes, 2 warps)
plus the bpp / PSNR reductions -- SURVEY.md 8(d).  Workload at N=1: BASELINE config C2 (batch 8, bf16 storage,
fp32 accumulation).  N>1: every rank runs its own batch of 8 (independent pairs, no collective on the path,
weak scaling); only the final timing max / pair count are reduced.

``--mode train`` (BASELINE config C3): a step is one training iteration on the rank's batch of 8 pairs -- zero_grad,
forward with quantisation noise, R-D loss, backward, in-place RCCL all-reduce of the flat gradient buffer (N > 1; bucketed,
overlapped with the backward pass), Adam, aux-loss backward, aux all-reduce, aux Adam (ywz/mywork/newtrain1.py:74-111) --
replayed from one HIP graph per rank (``--eager`` issues it from Python).  Weak scaling: global batch = 8 N.

A plain run sets up, warms up, times ``--steps`` steps, writes the last timed step's results if ``--dump-outputs DIR`` is given and
prints ONE JSON line (rank 0) with the contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step).  ``--full`` then
measures and checks the rest after the timed region and adds it to the line, among it
  roofline      dominant kernel (implicit-GEMM conv, bf16 MFMA): achieved TFLOP/s = algorithmic conv FLOPs of its
                launches / their summed HIP-event durations, measured live on the launch stream
  cpu_baseline  the CPU oracle (a port of the reference's forward, oracle/hesic_oracle.py) timed on this box's host
                cores on a bounded sample of the same workload (rank 0, N=1 only)
  parity        |bpp - bpp_oracle|, |PSNR - PSNR_oracle| averaged over the distinct pairs of the batch (and per pair): bf16 GPU path vs fp32 CPU oracle
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0     # dense bf16 = dense f16, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0              # HBM3E spec (the guide's measured copy ceiling is 6.29 TB/s)
HESIC_GFLOP_PER_PAIR_512 = 155.66
JOINT_GFLOP_PER_PAIR_512 = 126.2   # HESIC+, live masked taps (BASELINE.md section 2 / SURVEY 8d)


def gflop_per_pair(model, h, w):
    return (HESIC_GFLOP_PER_PAIR_512 if model == "hsic" else JOINT_GFLOP_PER_PAIR_512) * (h * w / 512 ** 2)


def conv_flops(B, Ho, Wo, H, W, Cin, Cout, k, transposed, ntaps=None):
    """FLOP = 2 x MAC; Conv2d: out_numel*Cin*k^2, ConvTranspose2d: in_numel*Cout*k^2."""
    taps = ntaps if ntaps is not None else k * k
    if transposed:
        return 2.0 * B * H * W * Cin * Cout * taps
    return 2.0 * B * Ho * Wo * Cin * Cout * taps


class KernelMeter:
    """One HIP event pair around every implicit-GEMM launch (hesic_conv2d_forward[_ws|_f32out] / hesic_conv2d_gdn_forward),
    recorded on the stream the kernel is launched on; the launch descriptor gives the algorithmic FLOPs and
    hesic_conv2d_variant names the instantiation the library picked."""
    NAMES = ("hesic_conv2d_forward", "hesic_conv2d_forward_ws", "hesic_conv2d_forward_f32out", "hesic_conv2d_gdn_forward", "hesic_conv2d_forward_grouped",
             "hesic_conv2d_forward_hilo", "hesic_conv2d_gdn_forward_hilo_out")

    STREAM = {"hesic_warp_perspective_forward": "warp_perspective", "hesic_sconv2d_gdn_forward": "conv1_3to128_gdn (n2w)",
              "hesic_sconv2d_gdn_forward_prepacked": "conv1_3to128_gdn (n2w)", "hesic_sconv2d_forward": "g_s_conv4_128to3 (w2n)",
              "hesic_sconv2d_forward_prepacked": "g_s_conv4_128to3 (w2n)", "hesic_sconv2d_gdn_forward_hilo": "conv1_3to128_gdn hi/lo (n2w, x3)",
              "hesic_sconv2d_gdn_forward_hilo_out1": "conv1_3to128_gdn hi/lo inside, single out (n2w, x3c2)"}

    def __init__(self, L):
        self.L, self.orig, self.rec, self.stream = L, L.call, [], {}

    def _stream_bytes(self, name, d):
        """ALGORITHMIC HBM bytes of one launch: every input element read once, every output element written once."""
        size = lambda dt: 2 if dt == self.L.H16 else 4
        if name == "hesic_warp_perspective_forward":
            return d.B * d.C * (d.H * d.W * size(d.src_dtype) + d.Ho * d.Wo * size(d.dst_dtype))
        if name.startswith("hesic_sconv2d_forward") and not (d.transposed and d.Cin >= 32):
            return None                       # only the 128 -> 3 synthesis output stage is priced here
        out_mult = 2 if name.endswith("_hilo") else 1            # [hi | lo] pairs: two bf16 per output value
        return d.B * (d.H * d.W * d.Cin * size(d.x_dtype) + d.Ho * d.Wo * d.Cout * size(d.y_dtype) * out_mult)

    def __enter__(self):
        def call(name, *args):
            if name in self.STREAM:
                nbytes = self._stream_bytes(name, args[0]._obj)
                if nbytes is None:
                    return self.orig(name, *args)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = self.orig(name, *args)
                e1.record()
                self.stream.setdefault(self.STREAM[name], []).append((e0, e1, nbytes))
                return rc
            if name not in self.NAMES:
                return self.orig(name, *args)
            d = args[0]._obj
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self.orig(name, *args)
            e1.record()
            ntaps = bin(d.tap_mask_lo).count("1") if d.tap_mask_lo else None
            fl = conv_flops(d.B, d.Ho, d.Wo, d.H, d.W, d.Cin, d.Cout, d.KH, d.transposed, ntaps)
            hilo = name.endswith("_hilo")
            fused = name.endswith("gdn_forward") or name.endswith("hilo_out") or (hilo and args[4] is not None and getattr(args[4], "value", None))
            if fused:
                fl += 2.0 * d.B * d.Ho * d.Wo * d.Cout * d.Cout          # the GDN 1x1 contraction (SURVEY 8d counts it)
            # a hi/lo (bf16x3) launch EXECUTES three bf16 MFMA products per algorithmic MAC: x_hi w_hi + x_lo w_hi + x_hi w_lo
            dv = d
            if hilo:                              # the tile choice of a hi/lo launch follows the packed K extent per tap, 2 Cin
                import copy
                dv = copy.copy(d)
                dv.Cin, dv.x_pix_stride = 2 * d.Cin, max(d.x_pix_stride, 2 * d.Cin)
            self.rec.append((e0, e1, fl, self.variant(dv, fused, hilo and not name.endswith("hilo_out")) + (" grouped" if name.endswith("grouped") else "") + (" hilo" if hilo else "") + (" hilo-gdn-out" if name.endswith("hilo_out") else ""),
                             3.0 if hilo else 1.0))
            return rc
        self.L.call = call
        return self

    def __exit__(self, *exc):
        self.L.call = self.orig

    def variant(self, d, fused, hilo_pairs=False):
        import ctypes as C
        v = (C.c_int32 * 4)()
        self.orig("hesic_conv2d_variant", C.byref(d), v)
        # the plan query runs the single-operand tile choice; the pair + GDN launch is promoted to the 256-pixel 8-wave tile when the grid is
        # large enough (csrc/conv_igemm.hip) -- name what actually runs
        if (hilo_pairs and fused and tuple(v[:3]) == (128, 128, 64) and v[3] == 1
                and not d.transposed and d.B * ((d.Ho * d.Wo + 255) // 256) >= 384):
            v[0] = 256
        if v[3] == 2:
            return f"igemm_tr4_kernel<{'gdn' if fused else 'plain'}>"
        if v[3]:
            return f"igemm_glds_kernel<{v[0]},{v[1]},{v[2]}{',gdn' if fused else ''}>"
        return f"igemm_conv_kernel<{'h16' if d.dtype == self.L.H16 else 'f32'},{v[1]}>"

    def summary(self):
        """Per kernel instantiation: launches, summed event time, algorithmic FLOPs; returns the dominant one."""
        torch.cuda.synchronize()
        agg = {}
        for e0, e1, f, name, mult in self.rec:
            a = agg.setdefault(name, [0, 0.0, 0.0, mult])
            a[0] += 1
            a[1] += e0.elapsed_time(e1) * 1e-3
            a[2] += f
        if not agg:
            return None
        name, (n, t, f, mult) = max(agg.items(), key=lambda kv: kv[1][1])
        streaming = {}
        for k, recs in self.stream.items():
            ts = sum(e0.elapsed_time(e1) for e0, e1, _ in recs) * 1e-3
            by = sum(r[2] for r in recs)
            streaming[k] = {"bound": "hbm", "achieved": round(by / ts / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(by / ts / 1e9 / HBM_PEAK_GBS, 4),
                            "launches": len(recs), "avg_launch_us": round(1e6 * ts / len(recs), 2), "bytes_per_launch": int(by / len(recs))}
        self.streaming = streaming
        # "tflops" = ALGORITHMIC (2 x MAC of the layer) over time, as the contract defines roofline.achieved; a hi/lo launch
        # executes three bf16 MFMA products per MAC, so its matrix-core rate is 3x that ("executed_tflops")
        return {"kernel": name, "launches": n, "avg_us": 1e6 * t / n, "tflops": f / t / 1e12, "flops_per_launch": f / n,
                "mfma_products_per_mac": mult, "executed_tflops": mult * f / t / 1e12,
                "all": {k: {"launches": v[0], "avg_us": round(1e6 * v[1] / v[0], 2), "tflops": round(v[2] / v[1] / 1e12, 1),
                            **({"executed_tflops": round(v[3] * v[2] / v[1] / 1e12, 1)} if v[3] != 1.0 else {})}
                        for k, v in agg.items()}}


class WgradMeter:
    """Training mode: one HIP event pair around the split-K MFMA launch of every wide weight gradient.  The training path
    issues ``hesic_conv2d_wgrad_direct`` (MFMA launch + finishing launch); during the metering pass each such call is
    preceded by ``hesic_conv2d_wgrad_partial`` -- the MFMA launch alone, same arguments, bracketed by the events."""

    def __init__(self, L):
        self.L, self.orig, self.rec = L, L.call, []

    def __enter__(self):
        def call(name, *args):
            if name == "hesic_conv2d_wgrad_direct":
                d = args[0]._obj
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.orig("hesic_conv2d_wgrad_partial", args[0], args[1], args[2], args[6], args[7], args[8])
                e1.record()
                ntaps = bin(d.tap_mask_lo).count("1") if d.tap_mask_lo else None
                self.rec.append((e0, e1, conv_flops(d.B, d.Ho, d.Wo, d.H, d.W, d.Cin, d.Cout, d.KH, d.transposed, ntaps), self.kernel_of(d)))
            if name == "hesic_conv2d_wgrad_partial":          # Trainer.step with the batched finishing pass: the MFMA launch is its own call
                d = args[0]._obj
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = self.orig(name, *args)
                e1.record()
                ntaps = bin(d.tap_mask_lo).count("1") if d.tap_mask_lo else None
                self.rec.append((e0, e1, conv_flops(d.B, d.Ho, d.Wo, d.H, d.W, d.Cin, d.Cout, d.KH, d.transposed, ntaps), self.kernel_of(d)))
                return rc
            if name == "hesic_conv2d_wgrad_partial_batched":
                # round 5: the split-K launches of a few queued layers in one call.  Row-kernel layers are launched one by one inside it: the
                # meter issues those itself (one event pair each, as above); the one-tap-per-block layers go down as ONE batched call -- the
                # shared grid is what the step runs -- under one event pair carrying the sum of their flops ("wgrad_tr_batched_kernel").
                import ctypes as C
                m, descs, xs, dys, wss, nbytes, nsp, st = args
                tr = []
                for i in range(m):
                    d = descs[i]
                    ntaps = bin(d.tap_mask_lo).count("1") if d.tap_mask_lo else None
                    fl = conv_flops(d.B, d.Ho, d.Wo, d.H, d.W, d.Cin, d.Cout, d.KH, d.transposed, ntaps)
                    if self.kernel_of(d) == "wgrad_row_kernel":
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        self.orig("hesic_conv2d_wgrad_partial", C.byref(d), C.c_void_p(xs[i]), C.c_void_p(dys[i]), C.c_void_p(wss[i]), nbytes[i], st)
                        e1.record()
                        self.rec.append((e0, e1, fl, "wgrad_row_kernel"))
                    else:
                        tr.append((i, fl))
                if tr:
                    k = len(tr)
                    vp = C.c_void_p * k
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    self.orig(name, k, (type(descs[0]) * k)(*[descs[i] for i, _ in tr]), vp(*[xs[i] for i, _ in tr]), vp(*[dys[i] for i, _ in tr]),
                              vp(*[wss[i] for i, _ in tr]), (C.c_int64 * k)(*[nbytes[i] for i, _ in tr]),
                              (C.c_int32 * k)(*[nsp[i] for i, _ in tr]) if nsp is not None else None, st)
                    e1.record()
                    self.rec.append((e0, e1, sum(f for _, f in tr), "wgrad_tr_batched_kernel"))
                    self.batched_layers = getattr(self, "batched_layers", 0) + k
                return None
            return self.orig(name, *args)
        self.L.call = call
        return self

    def __exit__(self, *exc):
        self.L.call = self.orig

    @staticmethod
    def kernel_of(d):
        """Which kernel csrc/wgrad.hip's fill_args gives this layer (round 5): the row kernel takes the 5x5 stride-2 layers whose pixel grid
        has rows of a multiple of 64 and >= 100 000 pixels (and HESIC_WGRAD_ROW != 0); everything else one tap per block."""
        qh, qw = (d.H, d.W) if d.transposed else (d.Ho, d.Wo)
        row = (os.environ.get("HESIC_WGRAD_ROW", "1") != "0" and d.KH == 5 and d.KW == 5 and d.stride == 2 and d.pad == 2 and not d.tap_mask_lo
               and not d.in_abs and qw % 64 == 0 and d.B * qh * qw >= int(os.environ.get("HESIC_WGRAD_ROW_MINQ", "100000")))
        return "wgrad_row_kernel" if row else "wgrad_tr_kernel"

    def summary(self):
        torch.cuda.synchronize()
        n = len(self.rec)
        if not n:
            return None
        t = sum(e0.elapsed_time(e1) for e0, e1, *_ in self.rec) * 1e-3
        f = sum(r[2] for r in self.rec)
        by = {}
        for e0, e1, fl, k in self.rec:
            b = by.setdefault(k, [0, 0.0, 0.0])
            b[0] += 1; b[1] += e0.elapsed_time(e1) * 1e-3; b[2] += fl
        return {"launches": n, "avg_us": 1e6 * t / n, "tflops": f / t / 1e12, "flops_per_launch": f / n,
                "by_kernel": {k: {"launches": v[0], "avg_us": round(1e6 * v[1] / v[0], 2), "tflops": round(v[2] / v[1] / 1e12, 2),
                                  "gflop_per_launch": round(v[2] / v[0] / 1e9, 3), "share_of_wgrad_time": round(v[1] / t, 4)} for k, v in by.items()}}


def cpu_train_baseline(kind, P_cpu, param_names, size, lmbda, budget_s=15.0):
    """One reference-order training step of the CPU oracle (forward with noise, R-D loss, backward, Adam, aux backward,
    aux Adam) on a bounded sample: 1 pair per step."""
    from hesic_amd import synthetic
    from oracle import hesic_oracle as O
    fwd = O.hsic_forward if kind == "hsic" else O.hsic_joint_forward
    cores = os.cpu_count() or 1
    torch.set_num_threads(min(16, cores))
    P = {k: v.clone() for k, v in P_cpu.items()}
    aux_keys = [k for k in param_names if k.startswith("entropy_bottleneck")]
    main_keys = [k for k in param_names if not k.startswith("entropy_bottleneck")]
    for k in param_names:
        P[k].requires_grad_()
    opt = torch.optim.Adam([P[k] for k in main_keys], lr=1e-4)
    aux = torch.optim.Adam([P[k] for k in aux_keys], lr=1e-3)
    x1, x2, Hm = synthetic.stereo_batch(0, 1, size, size)

    zs, ys = (1, 128, size // 64, size // 64), (1, 192, size // 16, size // 16)

    def step():
        opt.zero_grad(); aux.zero_grad()
        noise = {k: torch.empty(zs if k[0] == "z" else ys).uniform_(-0.5, 0.5) for k in ("z1", "y1", "y1b", "y1w", "z2", "y2", "y2b")}
        out = fwd(P, x1, x2, Hm, training=True, noise=noise)
        O.rd_loss(out, x1, x2, lmbda)["loss"].backward()
        opt.step()
        O.aux_loss(P).backward()
        aux.step()

    step()
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s or n >= 16:
            break
    return {"value": n / el, "unit": "stereo-pairs/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{n} training steps x (1 pair {size}x{size}, fp32, torch CPU autograd + Adam x2) after 1 warm-up, {el:.1f} s, "
                      f"{torch.get_num_threads()} of {cores} host cores"}


def cpu_baseline(kind, P_cpu, size, budget_s=12.0, parity_pairs=1):
    from hesic_amd import synthetic
    from oracle import hesic_oracle as O
    fwd = O.hsic_forward if kind == "hsic" else O.hsic_joint_forward
    cores = os.cpu_count() or 1
    # torch's CPU convs do not scale to hundreds of threads on this workload (256 threads measured 60x slower than
    # 8): calibrate the thread count on a 256x256 pair, then time the 512x512 sample with the best one
    xs1, xs2, Hs = synthetic.stereo_batch(0, 1, 256, 256)
    best_t, best = None, 1e30
    for nt in sorted({t for t in (8, 16, 32, 64) if t <= cores} or {cores}):
        torch.set_num_threads(nt)
        with torch.no_grad():
            fwd(P_cpu, xs1, xs2, Hs)
            t0 = time.perf_counter()
            fwd(P_cpu, xs1, xs2, Hs)
            dt = time.perf_counter() - t0
        if dt < best:
            best_t, best = nt, dt
    torch.set_num_threads(best_t)
    x1, x2, Hm = synthetic.stereo_batch(0, 1, size, size)
    with torch.no_grad():
        out = fwd(P_cpu, x1, x2, Hm)       # warm-up + the parity sample
        n, t0 = 0, time.perf_counter()
        while True:
            fwd(P_cpu, x1, x2, Hm)
            n += 1
            el = time.perf_counter() - t0
            if el > budget_s or n >= 64:
                break
    m = O.metrics(out, x1, x2)
    m["y_hat"] = {k: out[k].to(torch.int16) for k in ("y1_hat", "y2_hat")}      # rounded latents of the sample: the bit-exactness check
    if min(x1.shape[-2:]) > 160:
        m["ms_ssim"] = float((O.ms_ssim(out["x1_hat"], x1)[0] + O.ms_ssim(out["x2_hat"], x2)[0]) / 2)      # test3real.py:107-109
    if kind == "hsic":
        # the third analysis pass, round(encoder1(warp(x1_hat))) (newnet1.py:753-757): not transmitted, it conditions view 2's entropy
        # parameters; the product runs it on single 16-bit operands (error-feedback weights), so its flips are reported separately
        with torch.no_grad():
            m["y1_hat_w"] = torch.round(O.g_a(P_cpu, "encoder1.", O.warp_perspective(out["x1_hat"], Hm, x1.shape[-2:], True))).to(torch.int16)
    # the other distinct pairs of the timed batch: the parity block reports the set average the reference's own
    # evaluation reports (test3real.py:110-122) next to every pair
    m["more"] = []
    for j in range(1, parity_pairs):
        xa, xb, hh = synthetic.stereo_batch(j, 1, size, size)
        with torch.no_grad():
            oj = fwd(P_cpu, xa, xb, hh)
        mj = O.metrics(oj, xa, xb)
        mj["y_hat"] = {k: oj[k].to(torch.int16) for k in ("y1_hat", "y2_hat")}
        m["more"].append(mj)
    return {"value": n / el, "unit": "stereo-pairs/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{n} x (1 pair {size}x{size}, fp32, torch CPU ops) after 1 warm-up, {el:.1f} s; threads calibrated "
                      f"over 8/16/32/64 of {cores} host cores"}, m


def trained_parity(kind="hsic", sets=4, steps=3000, size=512, lr=1e-4, aux_lr=1e-3, lmbda=0.0067, log=None):
    """Parity at TRAINED operating points instead of the random-weight regime (bpp ~5.5, PSNR ~5.6 dB, likelihoods in the tails).
    No checkpoints exist offline, so ``sets`` models (weight salts 0..sets-1, their own training pairs) are trained here for
    ``steps`` graph-replayed steps on synthetic 256 x 256 pairs, which takes them to a low-rate / moderate-quality regime; each is
    then evaluated on pair 0 at ``size`` in the bf16 mode with both analysis precisions and in fp32, against the CPU oracle run
    on the SAME trained weights.  Returns one record per (set, mode)."""
    import hesic_amd
    from hesic_amd import functional as Fn, models, synthetic
    from hesic_amd.train import GraphedTrainer
    from oracle import hesic_oracle as O          # the checker (bench.py may: see oracle/hesic_oracle.py header)
    recs = []
    keep_dt, keep_an = Fn.compute_dtype(), Fn.analysis_precision()
    for sset in range(sets):
        hesic_amd.set_compute_dtype(torch.bfloat16)        # training runs in bf16
        net = (models.HSIC if kind == "hsic" else models.HSICJoint)()
        synthetic.fill_state_dict_(net.state_dict(), salt=sset)
        net = net.cuda()
        tr = GraphedTrainer(net, lr=lr, aux_lr=aux_lr, lmbda=lmbda)
        pool = [tuple(t.cuda() for t in synthetic.stereo_batch(100 + 1000 * sset + 8 * i, 8, 256, 256)) for i in range(16)]      # 128 distinct pairs
        for st in range(steps):
            c = tr.step(*pool[st % len(pool)])
            if log and (st % 1000 == 0 or st == steps - 1):
                log(f"# set {sset} step {st}: loss {float(c['loss']):.3f} bpp {float(c['bpp_loss']):.3f} mse {float(c['mse_loss']):.5f}")
        torch.cuda.synchronize()
        del tr
        net.eval()
        Fn.invalidate_weight_cache()
        P = {k: v.detach().float().cpu().clone() for k, v in net.state_dict().items()}
        x1, x2, Hm = synthetic.stereo_batch(0, 1, size, size)
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        with torch.no_grad():
            ref = (O.hsic_forward if kind == "hsic" else O.hsic_joint_forward)(P, x1, x2, Hm)
        mr = O.metrics(ref, x1, x2)
        for dt, an in ((torch.float16, "x3"), (torch.float16, "x3c2"), (torch.float16, "x1"), (torch.bfloat16, "x3"), (torch.bfloat16, "x1"), (torch.float32, None)):
            hesic_amd.set_compute_dtype(dt)
            Fn.invalidate_weight_cache()
            if an:
                Fn.set_analysis_precision(an)
            with torch.no_grad():
                out = net(x1.cuda(), x2.cuda(), Hm.cuda())
                m = models.metrics_from(models.rate_distortion(out, x1.cuda(), x2.cuda()))
            flips = {k: float((out[k].float().cpu() != ref[k]).float().mean()) for k in ("y1_hat", "y2_hat")}
            recs.append({"model": kind, "weight_set": sset, "trained_steps": steps, "eval": f"{size}x{size} pair 0",
                         "mode": "fp32" if dt == torch.float32 else f"{'f16' if dt == torch.float16 else 'bf16'} maps, analysis {an}",
                         "bpp_oracle": round(mr["bpp"], 5), "psnr_oracle": round(mr["psnr"], 4), "abs_dbpp": round(abs(m["bpp"] - mr["bpp"]), 6),
                         "rel_dbpp": round(abs(m["bpp"] - mr["bpp"]) / mr["bpp"], 6), "abs_dpsnr_db": round(abs(m["psnr"] - mr["psnr"]), 6),
                         "latent_flips": {k: round(v, 6) for k, v in flips.items()},
                         "nonzero_latents": round(float((ref["y1_hat"] != 0).float().mean()), 4)})
        del net
    hesic_amd.set_compute_dtype(keep_dt)
    Fn.set_analysis_precision(keep_an)
    return recs



def _timed_loop(fn, warm, n):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def secondary_modes(dev, oracle_pairs, size=512):
    """BASELINE config C2 (HESIC, 8 x 512^2) in the modes the headline is NOT run in, each with pairs/s and its parity triple against the
    same fp32 CPU oracle results the headline's ``parity`` block uses: bfloat16 maps with pair analysis (the dtype BASELINE.json names
    literally) and float16 "x3c2" (round 4's default, now an explicit fast mode -- its trained-point PSNR deviation is why)."""
    import hesic_amd
    from hesic_amd import functional as Fn, models, synthetic
    out = {}
    keep_dt, keep_an = Fn.compute_dtype(), Fn.set_analysis_precision("auto")
    try:
        npar = len(oracle_pairs)
        base = [synthetic.stereo_batch(j, 1, size, size) for j in range(npar)]
        x1, x2, Hm = (torch.cat([b[i] for b in base] * (8 // npar), 0).to(dev) for i in range(3))
        for name, dt, an in (("bf16_x3", torch.bfloat16, "x3"), ("f16_x3c2", torch.float16, "x3c2")):
            hesic_amd.set_compute_dtype(dt)
            Fn.set_analysis_precision(an)
            net = models.HSIC()
            synthetic.fill_state_dict_(net.state_dict())
            net = net.to(dev).eval()

            def fwd(i):
                with torch.no_grad():
                    return models.rate_distortion(net(x1, x2, Hm), x1, x2)
            ms = 1e3 * _timed_loop(fwd, 12, 30)
            per = []
            for j, mc in enumerate(oracle_pairs):
                with torch.no_grad():
                    oj = net(x1[j:j + 1], x2[j:j + 1], Hm[j:j + 1])
                    mj = models.metrics_from(models.rate_distortion(oj, x1[j:j + 1], x2[j:j + 1]))
                fl = max(float((oj[k].float().cpu().to(torch.int16) != v).float().mean()) for k, v in mc["y_hat"].items())
                per.append((mj["bpp"] - mc["bpp"], mj["psnr"] - mc["psnr"], fl))
            out[name] = {"value": round(8e3 / ms, 2), "unit": "stereo-pairs/s", "ms_per_step": round(ms, 3), "issue": "eager",
                         "parity": {"abs_dbpp": float("%.3g" % abs(sum(q[0] for q in per) / npar)), "abs_dpsnr_db": float("%.3g" % abs(sum(q[1] for q in per) / npar)),
                                    "latent_flips_worst_pair": float("%.3g" % max(q[2] for q in per)),
                                    "worst_pair_abs_dbpp": float("%.3g" % max(abs(q[0]) for q in per)), "pairs": npar}}
            del net
    except Exception as e:
        out["error"] = f"{type(e).__name__}: {e}"
    finally:
        hesic_amd.set_compute_dtype(keep_dt)
        Fn.set_analysis_precision(keep_an)
    return out


def secondary_sweep_and_path_a(dev, size=512, oracle_pairs=None):
    """BASELINE config C5 through ``evaluate.LambdaSweep`` (four lambda-models on 860 x 1080 pairs padded to 896 x 1088, B = 4 per step) for
    HESIC and HESIC+, and INTEGRATION.md path A -- the reference's own call order over the drop-in modules (``hesic_amd.path_a``), plain NCHW
    tensors between modules, no fused schedule -- for HESIC at 8 x 512^2: pairs/s each, in the headline's dtype."""
    import hesic_amd
    from hesic_amd import functional as Fn, models, path_a, synthetic
    from hesic_amd.evaluate import LambdaSweep
    out = {}
    try:
        x1, x2, Hm = (t.to(dev) for t in synthetic.stereo_batch(0, 4, 860, 1080))
        x1p, x2p = models.pad_to_multiple(x1), models.pad_to_multiple(x2)
        for kind in ("hsic", "joint"):
            sweep = LambdaSweep(kind, dev)
            ms = 1e3 * _timed_loop(lambda i: sweep.step(i % 4, x1, x2, x1p, x2p, Hm, True), 12, 16)
            gf = gflop_per_pair(kind, x1p.shape[-2], x1p.shape[-1])
            out["c5_sweep_" + ("hesic" if kind == "hsic" else "hesicplus")] = {
                "value": round(4e3 / ms, 2), "unit": "stereo-pairs/s", "ms_per_step": round(ms, 3), "pairs_per_step": 4, "padded": [int(x1p.shape[-2]), int(x1p.shape[-1])],
                "model_tflops": round(4 * gf / ms, 2), "mfma_frac_of_step": round(4 * gf / ms / MFMA_BF16_PEAK_TFLOPS, 4), "analysis": Fn.analysis_precision()}
            del sweep
        del x1, x2, x1p, x2p
        net = models.HSIC()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.to(dev).eval()
        a, b, h = (t.to(dev) for t in synthetic.stereo_batch(0, 8, size, size))

        def fwd_a(i):
            with torch.no_grad():
                return models.rate_distortion(path_a.hsic_forward(net, a, b, h), a, b)        # the same step as the headline: forward + bits / squared error
        ms = 1e3 * _timed_loop(fwd_a, 8, 20)
        rec = {"value": round(8e3 / ms, 2), "unit": "stereo-pairs/s", "ms_per_step": round(ms, 3), "issue": "eager, one stream",
               "analysis": Fn.analysis_precision(),
               "note": "the reference's call order (newnet1.py:724-783) over the drop-in compressai modules, every module's output handed to the next "
                       "as it is; round 6: the modules hand over among themselves at inference (hesic_amd/handover.py: deferred conv -> GDN fusion, "
                       "hi/lo pairs and fp32 latents between consecutive modules), HESIC_NO_HANDOVER=1 = round 5's literal launches; "
                       "parity bars: tests/test_gpu_path_a.py"}
        if oracle_pairs:
            per = []
            for j, mc in enumerate(oracle_pairs):
                with torch.no_grad():
                    oj = path_a.hsic_forward(net, a[j:j + 1], b[j:j + 1], h[j:j + 1])
                    mj = models.metrics_from(models.rate_distortion(oj, a[j:j + 1], b[j:j + 1]))
                fl = max(float((oj[k].float().cpu().to(torch.int16) != v).float().mean()) for k, v in mc["y_hat"].items())
                per.append((mj["bpp"] - mc["bpp"], mj["psnr"] - mc["psnr"], fl))
            npar = len(per)
            rec["parity"] = {"abs_dbpp": float("%.3g" % abs(sum(q[0] for q in per) / npar)), "abs_dpsnr_db": float("%.3g" % abs(sum(q[1] for q in per) / npar)),
                             "latent_flips_worst_pair": float("%.3g" % max(q[2] for q in per)),
                             "worst_pair_abs_dbpp": float("%.3g" % max(abs(q[0]) for q in per)), "pairs": npar}
        out["path_a_hesic_b8"] = rec
        del net
    except Exception as e:
        out["error"] = f"{type(e).__name__}: {e}"
    return out


EN_GFLOP_PER_PAIR_512 = 176.7          # Independent_EN: 2 views x (6*32*9 + 18*32*32*9 + 32*3*9) MAC per pixel x 512^2 x 2 (newnet1.py:272-311)


def secondary_hesic_en(dev, size=512):
    """What the published evaluation runs (ywz/mywork/test3real.py:186): HSIC followed by Independent_EN (newnet1.py:1278-1321) on 8 x 512^2
    pairs in the headline's mode -- pairs/s of the whole pipeline, the enhancement stage alone, and its dominant kernel (one ResidualBlock
    per launch, csrc/enh.hip) against the MFMA roofline by HIP events on the launch stream."""
    import hesic_amd
    from hesic_amd import _lib as L_, functional as Fn, models, synthetic
    out = {}
    try:
        net = models.GMM_together()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.to(dev).eval()
        a, b, h = (t.to(dev) for t in synthetic.stereo_batch(0, 8, size, size))

        def fwd(i):
            with torch.no_grad():
                return models.rate_distortion(net(a, b, h), a, b)
        ms = 1e3 * _timed_loop(fwd, 8, 20)
        with torch.no_grad():
            o1 = net.m1(a, b, h)
            x1h, x2h = o1["x1_hat"].float(), o1["x2_hat"].float()

            def en(i):
                return net.m2(x1h, x2h, h)
            ms_en = 1e3 * _timed_loop(en, 5, 20)
            # the ResidualBlock launches between HIP events on their stream (9 per view)
            orig, recs = L_.call, []

            def call(name, *args):
                if name not in ("hesic_resblock_c32_forward", "hesic_conv3x3_c32_forward"):
                    return orig(name, *args)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = orig(name, *args)
                e1.record()
                recs.append((name, e0, e1))
                return rc
            L_.call = call
            try:
                for _ in range(3):
                    net.m2(x1h, x2h, h)
            finally:
                L_.call = orig
            torch.cuda.synchronize()
        px = 8 * size * size
        per = {}
        for name, e0, e1 in recs:
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e-3)
        gf_en = EN_GFLOP_PER_PAIR_512 * (size * size / 512 ** 2)
        gf_all = gf_en + gflop_per_pair("hsic", size, size)
        out = {"value": round(8e3 / ms, 2), "unit": "stereo-pairs/s", "ms_per_step": round(ms, 3), "pairs_per_step": 8,
               "workload": "HSIC -> Independent_EN (GMM_together, newnet1.py:1304-1321) + bpp / PSNR of the enhanced reconstructions, 8 x 512^2, "
                           "headline dtype / analysis mode", "gflop_per_pair": round(gf_all, 1), "model_tflops": round(8 * gf_all / ms, 2),
               "mfma_frac_of_step": round(8 * gf_all / ms / MFMA_BF16_PEAK_TFLOPS, 4),
               "independent_en_alone": {"ms": round(ms_en, 3), "gflop_per_pair": round(gf_en, 1), "tflops": round(8 * gf_en / ms_en, 1),
                                        "frac": round(8 * gf_en / ms_en / MFMA_BF16_PEAK_TFLOPS, 4)}}
        rb = per.get("hesic_resblock_c32_forward")
        if rb:
            fl = 2.0 * px * 2 * 32 * 32 * 9          # two 32 -> 32 3x3 convs per launch
            t = sum(rb) / len(rb)
            out["roofline"] = {"kernel": "c32_resblock_r3_kernel", "bound": "mfma", "achieved": round(fl / t / 1e12, 2), "peak": MFMA_BF16_PEAK_TFLOPS,
                               "unit": "TFLOP/s", "frac": round(fl / t / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4), "launches_per_step": len(rb) // 3,
                               "avg_launch_us": round(1e6 * t, 2), "gflop_per_launch": round(fl / 1e9, 2),
                               "hbm_bytes_algorithmic": 2 * px * 64 + (px * 64), "traffic": None}
        cv = per.get("hesic_conv3x3_c32_forward")
        if cv:
            out["conv3x3_c32_avg_us"] = round(1e6 * sum(cv) / len(cv), 2)
        del net
    except Exception as e:
        out["error"] = f"{type(e).__name__}: {e}"
    return out


def secondary_train_rccl(dev, size=512, lmbda=0.0067):
    """The graph-replayed training step with a ONE-RANK RCCL process group in the graph (the bucketed all-reduces of config C3 run for real,
    over no link): what the collectives cost a step before any xGMI hop.  Runs as a CHILD process with a time limit (``bench.py --mode train``
    with HESIC_FORCE_COLLECTIVES=1): a collective library that fails to come up on some box must not take the headline line with it."""
    import subprocess
    env = dict(os.environ, HESIC_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", "train", "--steps", "12", "--warmup", "6", "--full", "--no-cpu-baseline", "--lmbda", str(lmbda), "--size", str(size)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"child exited with {r.returncode}: {(r.stderr or '').strip()[-300:]}"}
        d = json.loads(lines[-1])
        comm = d.get("comm") or {}
        return {"ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"], "dtype": d.get("dtype", "bf16"), "world_size": 1,
                "buckets": len(comm.get("buckets", []) or []), "comm_total_ms": comm.get("allreduce_total_ms"), "comm_hidden_frac": comm.get("hidden_under_backward_frac"),
                "per_bucket": [{"mb": b.get("mb"), "ms": b.get("ms")} for b in (comm.get("buckets") or [])],
                "step": "HIP graph replay with the RCCL all-reduces inside (child process)"}
    except subprocess.TimeoutExpired:
        return {"error": "child process exceeded 240 s"}
    except Exception as e:
        return {"error": f"{type(e).__name__}: {e}"}


def secondary_block(dev, size=512, lmbda=0.0067):
    """Two more driver-visible numbers, measured AFTER the headline's timed region (rank 0 of a 1-GPU run, a few seconds):
    BASELINE config C4 (HESIC+, 4 pairs of 512 x 512, the headline's dtype / analysis mode, eager issue) with its dominant conv kernel's
    roofline fraction, and one graph-replayed TRAINING step of HESIC at B=8 512 x 512 in bf16 (the per-GPU share of config C3)."""
    import hesic_amd
    from hesic_amd import _lib as L_, functional as Fn, models, synthetic
    from hesic_amd.train import GraphedTrainer
    out = {}
    keep = Fn.compute_dtype()
    try:
        # ---- C4
        net = models.HSICJoint()
        synthetic.fill_state_dict_(net.state_dict())
        net = net.to(dev).eval()
        xs = [tuple(t.to(dev) for t in synthetic.stereo_batch(4 * j, 4, size, size)) for j in range(4)]

        def fwd(i):
            a, b, h = xs[i % 4]
            with torch.no_grad():
                o = net(a, b, h)
                return models.rate_distortion(o, a, b)
        def timed(fn, n=40):
            for i in range(15):
                fn(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                fn(i)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        n = 40
        el_eager = timed(fwd, n)
        # at 4 pairs the GPU needs about as long as the host takes to issue ~75 launches: a whole-forward HIP graph is timed beside eager
        # issue and the faster of the two is the figure (the headline's --exec auto rule)
        graphed = models.GraphedForward(net, *xs[0], with_metrics=False)

        def fwd_graph(i):
            a, b, h = xs[i % 4]
            o, _ = graphed(a, b, h)
            with torch.no_grad():
                return models.rate_distortion(o, a, b)
        el_graph = timed(fwd_graph, n)
        del graphed
        el, issue = (el_graph, "graph") if el_graph < el_eager else (el_eager, "eager")
        overlap, models.OVERLAP_STREAMS = models.OVERLAP_STREAMS, False
        with KernelMeter(L_) as km:
            for i in range(3):
                fwd(i)
            s = km.summary()
        models.OVERLAP_STREAMS = overlap
        gf = gflop_per_pair("joint", size, size)
        out["c4_hesicplus_b4"] = {"value": round(4 * n / el, 2), "unit": "stereo-pairs/s", "ms_per_step": round(1e3 * el / n, 3), "pairs_per_step": 4,
                                  "issue": issue, "issue_ms": {"eager": round(1e3 * el_eager / n, 3), "graph": round(1e3 * el_graph / n, 3)},
                                  "dtype": {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[keep],
                                  "analysis": Fn.analysis_precision() if keep != torch.float32 else "fp32",
                                  "model_tflops": round(4 * n * gf / el / 1e3, 2), "gflop_per_pair": gf,
                                  "roofline": None if not s else {"kernel": s["kernel"], "bound": "mfma", "achieved": round(s["tflops"], 2), "peak": MFMA_BF16_PEAK_TFLOPS,
                                                                  "unit": "TFLOP/s", "frac": round(s["tflops"] / MFMA_BF16_PEAK_TFLOPS, 4),
                                                                  "avg_launch_us": round(s["avg_us"], 2), "launches_per_step": s["launches"] // 3}}
        del net, xs
        # ---- one training step (C3's per-GPU share), bf16, HIP-graph replay
        hesic_amd.set_compute_dtype(torch.bfloat16)
        tnet = models.HSIC()
        synthetic.fill_state_dict_(tnet.state_dict())
        tnet = tnet.to(dev).train()
        tr = GraphedTrainer(tnet, lr=1e-4, aux_lr=1e-3, lmbda=lmbda)
        x1, x2, Hm = (t.to(dev) for t in synthetic.stereo_batch(0, 8, size, size))
        for _ in range(tr.warmup + 3):
            tr.step(x1, x2, Hm)
        torch.cuda.synchronize()
        n, t0 = 12, time.perf_counter()
        for _ in range(n):
            crit = tr.step(x1, x2, Hm)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        gf3 = 3 * gflop_per_pair("hsic", size, size)
        out["train_step_hesic_b8"] = {"ms_per_step": round(1e3 * el / n, 3), "value": round(8 * n / el, 2), "unit": "stereo-pairs/s", "dtype": "bf16",
                                      "step": "HIP graph replay" if getattr(tr, "capturable", True) else "eager",
                                      "model_tflops": round(8 * n * gf3 / el / 1e3, 2),
                                      "mfma_frac_of_step": round(8 * n * gf3 / el / 1e3 / MFMA_BF16_PEAK_TFLOPS, 4),
                                      "loss_last_step": round(float(crit["loss"]), 4)}
        del tr, tnet
    except Exception as e:          # the headline must not die with the extras
        out["error"] = f"{type(e).__name__}: {e}"
    finally:
        hesic_amd.set_compute_dtype(torch.bfloat16 if keep == torch.float32 else keep)
        hesic_amd.set_compute_dtype(keep)
    return out


def _smi_sample():
    """Shader clock (MHz) and socket power (W) of the visible GPU from rocm-smi (the hwmon nodes inside the container belong to other cards)."""
    import subprocess
    try:
        out = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=10).stdout
        card = next(iter(json.loads(out).values()))
    except Exception:
        return None
    r = {}
    for k, v in card.items():
        kl = k.lower()
        if "sclk" in kl and "(" in str(v):
            try:
                r["sclk_mhz"] = float(str(v).split("(")[1].lower().split("mhz")[0])
            except ValueError:
                pass
        elif "power" in kl and "max" not in kl and "cap" not in kl:
            try:
                r["power_w"] = float(v)
            except (TypeError, ValueError):
                pass
    return r or None


def under_load(fn, seconds=2.0):
    """Run fn() back to back for `seconds` while a thread samples rocm-smi: the clock and socket power the chip settles at under that load
    (first half of the samples dropped).  Returns (calls made, wall seconds, {"sclk_mhz", "power_w", "samples"} or None)."""
    import threading
    samples, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            r = _smi_sample()
            if r:
                samples.append(r)
            time.sleep(0.02)
    th = threading.Thread(target=poll, daemon=True)
    torch.cuda.synchronize()
    th.start()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            fn()
        n += 4
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    stop.set()
    th.join(timeout=15)
    tail = samples[len(samples) // 2:]
    st = None
    if tail:
        st = {"samples": len(tail)}
        for k in ("sclk_mhz", "power_w"):
            v = [x[k] for x in tail if k in x]
            if v:
                st[k] = round(sum(v) / len(v), 1)
    return n, wall, st


def power_state(step_fn, dtype, dev):
    """`roofline.power_state`: what the board's power management does to the peak the roofline is priced against.  (a) the timed step replayed
    for 2 s, (b) a register-only MFMA loop (hesic_probe_mfma_loop: no LDS, no memory) on random and on all-zero operands, each with the clock and
    socket power rocm-smi reports meanwhile.  Measured AFTER the timed region; a report block, never the reason a run fails."""
    import ctypes as C
    from hesic_amd import _lib as L
    out = {"power_cap_w": 1400.0, "nominal_sclk_mhz": 2400.0, "how": "rocm-smi --showclocks --showpower polled from a thread while the load repeats for 2 s"}
    n, wall, st = under_load(step_fn)
    out["timed_step"] = dict(st or {}, ms_per_step=round(1e3 * wall / n, 3))
    h16 = torch.float16 if dtype == "f16" else torch.bfloat16
    sink = torch.zeros(1024, device=dev)
    for kind in ("random", "zeros"):
        src = ((torch.rand(32768, device=dev) - 0.5) * 0.25 if kind == "random" else torch.zeros(32768, device=dev)).to(h16)
        fl = C.c_double(0.0)

        def loop():
            L.call("hesic_probe_mfma_loop", L.ptr(src), L.ptr(sink), 2048, C.byref(fl), L.stream())
        loop()
        n, wall, st = under_load(loop, 1.5)
        out[f"mfma_loop_{kind}_operands"] = dict(st or {}, tflops=round(fl.value * n / wall / 1e12, 1))
    out["note"] = ("`peak` above is the nominal dense rate at 2.4 GHz; on random operands the matrix pipe alone holds mfma_loop_random_operands.tflops because the chip "
                   "leaves its nominal clock at the power cap, and the timed step runs at timed_step.sclk_mhz / power_w (profiles/r06_power_probe.txt: the dominant "
                   "launch alone sits AT the cap)")
    return out


def emit_line(obj):
    """The run's ONE JSON line, as the LAST thing on stdout: whatever native libraries have queued on the C stdio buffer (RCCL's
    NCCL_DEBUG=VERSION banner, which this image exports) is flushed first, then the line, flushed."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.write(json.dumps(obj) + "\n")
    sys.stdout.flush()


DUMP_BUDGET_BYTES = 60 * 10 ** 6        # --dump-outputs: under 64 MB in all


def flat_outputs(out, rd=None):
    """The arrays a caller of the forward receives (reconstructions, rounded latents, likelihoods) and, if given, the bits / squared-error
    sums of ``models.rate_distortion``, as one flat {name: tensor}."""
    arrays = {}
    for k, v in out.items():
        if isinstance(v, dict):
            arrays.update({f"{k}_{kk}": vv for kk, vv in v.items()})
        elif torch.is_tensor(v):
            arrays[k] = v
    for k, v in (rd or {}).items():
        if torch.is_tensor(v):
            arrays["rd_" + k] = v
    return arrays


def dump_outputs(path, arrays, seed=0):
    """--dump-outputs: write every array as ``path/<name>.npy`` -- float64 where the path computes fp64 (the rate / distortion sums), float32
    otherwise.  The arrays share DUMP_BUDGET_BYTES: the small ones are written whole, an array larger than its share is replaced by the 1-D
    sample of its flattened elements at positions drawn by a generator seeded with ``seed`` (sorted, the same on every run of the same
    arguments)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        t = t.detach()
        host[name] = t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()
    left, budget = len(host), DUMP_BUDGET_BYTES
    for name in sorted(host, key=lambda k: host[k].nbytes):
        a = host[name]
        cap = (budget // left) // a.itemsize
        if a.size > cap:
            idx = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(a.size, size=cap, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))
        budget -= a.nbytes
        left -= 1


def sweep_main(args, batch, rank, world, dev, H_img, W_img):
    """--sweep: BASELINE config C5.  Four lambda-models (four independent weight sets; there are no trained checkpoints
    offline, so four deterministic synthetic fills), InStereo2K-size pairs zero-padded to x64, reconstructions cropped, bpp
    over the original pixels (``hesic_amd.evaluate.LambdaSweep``).  Every rank evaluates one (model, batch) unit per step; the
    model index rotates over ranks and steps, so all four are exercised on any N.  No collective on the path; per-lambda sums
    are reduced once at the end."""
    import torch.distributed as dist
    from hesic_amd.evaluate import SWEEP_LAMBDAS, LambdaSweep
    x1, x2, x1p, x2p, Hm = batch
    sweep = LambdaSweep(args.model, dev)
    acc = sweep.acc

    def step(k, record):
        return sweep.step((rank + k) % 4, x1, x2, x1p, x2p, Hm, record)

    for k in range(max(args.warmup, 12)):          # three rounds: every model packs its weights, the allocator pools settle, and the
        step(k, True)                              # accumulation ops are loaded too (their first launches cost ~60 ms in all)
    acc.zero_()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        last = step(k, True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed, ranks_info = job_time(elapsed, world, dev, args.batch * args.steps)
    if world > 1:
        dist.all_reduce(acc)
    if rank == 0 and args.dump_outputs and args.steps > 0:
        dump_outputs(args.dump_outputs, dict(flat_outputs(*last), lambda_sums=acc))
    if rank == 0:
        pairs = world * args.batch * args.steps
        per = {lam: {"pairs": v["pairs"], "bpp": round(v["bpp"], 5), "psnr": round(v["psnr"], 4)} for lam, v in sweep.summary(H_img, W_img).items()}
        # dominant conv kernel of the sweep's steps, measured live after the timed region (single stream: an event pair brackets ONE kernel)
        from hesic_amd import _lib as L_, models as models_
        roof, s = None, None
        if args.full:
            overlap, models_.OVERLAP_STREAMS = models_.OVERLAP_STREAMS, False
            with KernelMeter(L_) as km:
                for k in range(4):
                    step(k, False)
                s = km.summary()
            models_.OVERLAP_STREAMS = overlap
        if s:
            peak = MFMA_BF16_PEAK_TFLOPS if args.dtype != "f32" else MFMA_F32_PEAK_TFLOPS
            roof = {"kernel": s["kernel"], "bound": "mfma", "achieved": round(s["tflops"], 2), "peak": peak, "unit": "TFLOP/s", "frac": round(s["tflops"] / peak, 4),
                    "traffic": None, "mfma_products_per_mac": s["mfma_products_per_mac"], "launches_per_step": s["launches"] // 4, "avg_launch_us": round(s["avg_us"], 2),
                    "gflop_per_launch": round(s["flops_per_launch"] / 1e9, 3), "streaming_kernels": km.streaming}
        emit_line({
            "metric": "stereo-pairs/sec encode+decode @512x512; bpp & PSNR delta vs reference",
            "value": round(pairs / elapsed, 2), "unit": "stereo-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic", "full": args.full,
            "config": {"workload": f"BASELINE config C5: {'HESIC' if args.model == 'hsic' else 'HESIC+'} rate-distortion sweep, 4 lambda-models x "
                                   f"{H_img}x{W_img} pairs (zero-padded to {x1p.shape[-2]}x{x1p.shape[-1]}, bpp over the original pixels), batch {args.batch}/GPU",
                       "pairs_per_step": world * args.batch, "sharding": f"one (lambda-model, batch) unit per rank and step over {world} GPU(s), no collective on the path",
                       "lambdas": list(SWEEP_LAMBDAS)},
            "model_tflops": round(pairs * gflop_per_pair(args.model, x1p.shape[-2], x1p.shape[-1]) / elapsed / 1e3, 2),
            "per_lambda": per, "roofline": roof, "cpu_baseline": None, **({"ranks": ranks_info} if ranks_info else {})})
    if world > 1:
        dist.destroy_process_group()


def train_main(args, net, P_cpu, batch, rank, world, dev, H_img, W_img):
    """--mode train: see the module docstring.  Timed region = ``steps`` calls of ``Trainer.step`` on resident inputs."""
    import torch.distributed as dist
    from hesic_amd import _lib as L_, functional as Fn
    from hesic_amd.train import GraphedTrainer, Trainer
    x1, x2, Hm = batch
    net.train()
    param_names = [n for n, _ in net.named_parameters()]
    force = False
    if world == 1 and os.environ.get("HESIC_FORCE_COLLECTIVES"):
        # 1-GPU box: a one-rank RCCL group, so that the bucketed all-reduces (and the ``comm`` diagnostics below) run for real
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if not dist.is_initialized():
            dist.init_process_group("nccl", rank=0, world_size=1)
        force = True
    tr = (Trainer if args.eager else GraphedTrainer)(net, lr=1e-4, aux_lr=1e-3, lmbda=args.lmbda, force_collectives=force)
    for _ in range(max(args.warmup, 0 if args.eager else tr.warmup + 1)):
        crit = tr.step(x1, x2, Hm)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        crit = tr.step(x1, x2, Hm)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed, ranks_info = job_time(elapsed, world, dev, args.batch * args.steps)
    losses = {k: float(v) for k, v in crit.items()}
    if rank == 0 and args.dump_outputs and args.steps > 0:
        # what the step hands back (its loss terms) and what it leaves behind (the updated parameters, flattened in named_parameters order)
        dump_outputs(args.dump_outputs, dict({"loss_" + k: v.reshape(1) for k, v in crit.items() if torch.is_tensor(v)},
                                             parameters=torch.cat([p.detach().float().reshape(-1) for p in net.parameters()])))

    # roofline of the weight-gradient MFMA kernel, measured live (eager steps, events on the launch stream); launch census.
    # EVERY rank runs these extra steps (a step contains the gradient collectives: a rank that skipped them would hang the
    # others); only rank 0's events are reported.
    roof, census, s = None, {}, None
    eager = Trainer.step          # the un-graphed step of the same trainer object
    orig_call = L_.call

    def counting(name, *a):
        census[name] = census.get(name, 0) + 1
        return orig_call(name, *a)
    if args.full:
        L_.call = counting
        try:
            eager(tr, x1, x2, Hm)
        finally:
            L_.call = orig_call
        with WgradMeter(L_) as wm:
            for _ in range(2):
                eager(tr, x1, x2, Hm)
            s = wm.summary()
    if s and rank == 0:
        peak = MFMA_BF16_PEAK_TFLOPS if args.dtype != "f32" else MFMA_F32_PEAK_TFLOPS
        # the dominant kernel of the step by time is the weight-gradient family; since round 5 it has two members -- the line's figure is
        # the one with the larger share of the family's time, `wgrad_kernels` gives both (launch counts are per metering pass of 2 steps)
        byk = s["by_kernel"]
        top = max(byk, key=lambda k: byk[k]["share_of_wgrad_time"])
        roof = {"kernel": top, "bound": "mfma", "achieved": byk[top]["tflops"], "peak": peak, "unit": "TFLOP/s",
                "frac": round(byk[top]["tflops"] / peak, 4), "traffic": None, "launches_per_step": byk[top]["launches"] // 2,
                "avg_launch_us": byk[top]["avg_us"], "gflop_per_launch": byk[top]["gflop_per_launch"],
                "wgrad_kernels": {k: dict(v, frac=round(v["tflops"] / peak, 4)) for k, v in byk.items()},
                "wgrad_family": {"achieved": round(s["tflops"], 2), "frac": round(s["tflops"] / peak, 4), "launches_per_step": s["launches"] // 2,
                                 "avg_launch_us": round(s["avg_us"], 2)}}
        if getattr(wm, "batched_layers", 0) and "wgrad_tr_batched_kernel" in roof["wgrad_kernels"]:
            # one "launch" of this entry = one hesic_conv2d_wgrad_partial_batched call = the shared grid(s) of several layers
            roof["wgrad_kernels"]["wgrad_tr_batched_kernel"]["layers_per_step"] = wm.batched_layers // 2
    # gradient all-reduce, self-diagnosing (N > 1 on RCCL): ONE eager step whose buckets run synchronously on a communication stream
    # between events -- per-bucket duration, bus bandwidth and the share of the communication hidden under the backward pass
    comm = None
    if args.full and tr.main_reducer.active and tr.main_reducer.avg_op:
        from hesic_amd.train import comm_report
        tr.main_reducer.timing = True
        eager(tr, x1, x2, Hm)
        tr.main_reducer._timed.clear()               # first timed step: stream creation / RCCL channel set-up
        eager(tr, x1, x2, Hm)
        rep = comm_report(tr.main_reducer)
        tr.main_reducer.timing = False
        nb = len(rep["buckets"])
        comm = {"backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(), "gradient_mb": round(tr.main_group.numel * 4 / 1e6, 1),
                "buckets": rep["buckets"], "allreduce_total_ms": rep["total_ms"], "hidden_under_backward_frac": rep["hidden_frac"],
                "ring_busbw_gbps": round(2 * (world - 1) / world * tr.main_group.numel * 4 / 1e6 / max(rep["total_ms"], 1e-6), 1) if nb else None,
                "note": "one eager step, every bucket's all-reduce synchronous on its own stream between HIP events (rank 0's view)"}
    if world > 1:
        dist.barrier()

    # clock / socket power while the timed step repeats (after the timed region; one rank: the sample is the whole board's)
    pstate = None
    if args.full and world == 1 and not getattr(args, "no_power_state", False):
        try:
            n_, wall_, st_ = under_load(lambda: tr.step(x1, x2, Hm), 2.0)
            pstate = dict(st_ or {}, ms_per_step=round(1e3 * wall_ / n_, 3), power_cap_w=1400.0, nominal_sclk_mhz=2400.0,
                          how="rocm-smi --showclocks --showpower polled from a thread while the step repeats for 2 s")
        except Exception as e:
            print(f"# power_state skipped: {e}", file=sys.stderr)
    if rank == 0:
        pairs = world * args.batch * args.steps
        gflop_pair = 3 * HESIC_GFLOP_PER_PAIR_512 * (x1.shape[-2] * x1.shape[-1] / 512 ** 2)      # fwd + dgrad + wgrad
        res = {
            "metric": "stereo-pairs/sec encode+decode @512x512; bpp & PSNR delta vs reference",
            "value": round(pairs / elapsed, 2), "unit": "stereo-pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "full": args.full,
            "config": {"workload": f"{'HESIC' if args.model == 'hsic' else 'HESIC+'} TRAINING step (BASELINE config C3: R-D loss, Adam x2, "
                                   f"gradient all-reduce), {H_img}x{W_img} stereo pairs, batch {args.batch}/GPU, lambda {args.lmbda}",
                       "pairs_per_step": world * args.batch, "global_batch": world * args.batch,
                       "sharding": f"data parallel over {world} GPU(s): one in-place bucketed RCCL all-reduce of the "
                                   f"{tr.main_group.numel * 4 / 1e6:.1f} MB flat gradient per step" + ("" if world > 1 else " (single rank: no collective)"),
                       "step": "eager" if (args.eager or not getattr(tr, "capturable", True)) else "HIP graph replay"},
            "model_tflops": round(pairs * gflop_pair / elapsed / 1e3, 2) if args.model == "hsic" else None,
            "mfma_frac_of_step": round(pairs * gflop_pair / elapsed / 1e3 / world / MFMA_BF16_PEAK_TFLOPS, 4) if args.model == "hsic" and args.dtype != "f32" else None,
            "roofline": roof, "power_state_timed_step": pstate,
            "comm": comm,
            "launches_per_step": {"c_abi_calls": sum(census.values()), "note": "C-ABI calls of one eager step (each is 1-2 kernel launches); "
                                  "ATen launches not included -- see profiles/ for the rocprofv3 count"} if args.full else None,
            "losses_last_step": {k: round(v, 5) for k, v in losses.items()},
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            base = cpu_train_baseline(args.model, P_cpu, param_names, 512 if (args.height or args.width) else args.size, args.lmbda)
            res["cpu_baseline"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in base.items()}
        else:
            res["cpu_baseline"] = None
        if ranks_info is not None:
            ranks_info["gradient_collective"] = getattr(tr.main_reducer, "collective", "allreduce")
            res["ranks"] = ranks_info
        emit_line(res)
    if world > 1 or force:
        dist.destroy_process_group()


def job_time(elapsed, world, dev, units_per_rank, unit="pairs_per_s"):
    """(the job's time = the slowest rank's, a `ranks` block for the JSON line): every rank's own wall time of the timed region is gathered,
    and the communicator says what it is (backend `nccl` = RCCL on ROCm) and how many ranks it holds."""
    if world == 1:
        return elapsed, None
    import torch.distributed as dist
    mine = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    every = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    per_rank = [float(v) for v in every]
    return max(per_rank), {"backend": dist.get_backend(), "nranks": dist.get_world_size(),
                           "per_rank_" + unit: [round(units_per_rank / v, 1) for v in per_rank]}


def self_launch(n, argv=None):
    """Re-run this command line as ``n`` ranks of ONE node: ``python -m torch.distributed.run --nnodes=1 --nproc-per-node n
    --master-addr 127.0.0.1 --master-port <free port> bench.py <same flags>``.  Returns the job's exit code."""
    import socket
    import subprocess
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *(sys.argv[1:] if argv is None else argv)]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)      # >= 0.5 s of timed region at the default workload
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8, help="stereo pairs per GPU per step")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=None, help="non-square workloads (e.g. 860x1080, zero-padded to x64)")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--model", choices=["hsic", "joint"], default="hsic")
    ap.add_argument("--dtype", choices=["f16", "bf16", "f32"], default=None,
                    help="storage / matrix-core operand type of the wide maps (fp32 accumulation always).  Inference default f16: IEEE half runs at "
                         "the bf16 MFMA rate on gfx950 with 3 more significand bits (libhesic_hip_f16.so); training default bf16")
    ap.add_argument("--mode", choices=["infer", "train"], default="infer", help="train: BASELINE config C3 (R-D training step, DP gradient all-reduce)")
    ap.add_argument("--eager", action="store_true", help="train mode: issue the step from Python instead of replaying the HIP graph")
    ap.add_argument("--lmbda", type=float, default=0.0067)
    ap.add_argument("--sweep", action="store_true", help="BASELINE config C5: 4 lambda-models x pairs at --height/--width (default 860x1080), "
                    "one (model, batch) unit per rank and step, models rotating over ranks and steps")
    ap.add_argument("--warp-align-corners", type=int, choices=[0, 1], default=None,
                    help="0: kornia <= 0.4 sampling (what torch-1.6-era checkpoints were trained with), 1: kornia >= 0.5 (default)")
    ap.add_argument("--analysis", choices=["x1", "x3", "x3c2", "bf16", "bf16x3"], default=None,
                    help="operand precision of the analysis transforms + hyper-analysis at 16-bit inference: x3 = hi/lo pairs everywhere (three "
                         "products per MAC, fp32-grade latents), x3c2 = pairs except g_a_conv2 (70 %% of g_a's MACs) on single operands, x1 = single "
                         "operands (bf16 / bf16x3: the round-3 names of x1 / x3)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: the roofline of the dominant kernel (and the power state, the "
                         "launch census, the gradient all-reduce in train mode), the CPU oracle baseline with the parity against it, and the "
                         "`secondary` block.  A plain run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, at most 64 MB "
                         "in all; a larger array is written as a fixed, seeded sample of its elements).  Inputs are the same on every run")
    ap.add_argument("--parity-trained", type=int, default=0, metavar="SETS",
                    help="with --full: also report parity at TRAINED operating points: train SETS weight sets for --parity-train-steps steps each on synthetic "
                         "pairs (about 25 s per set) and compare bf16x3 / bf16 / fp32 against the CPU oracle on the trained weights")
    ap.add_argument("--parity-train-steps", type=int, default=3000)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline and the parity block")
    ap.add_argument("--no-power-state", action="store_true", help="with --full: skip roofline.power_state (clock / socket power under the timed step and under a matrix-only loop, ~6 s)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the `secondary` block (HESIC+ B=4 and one training step, ~5 s, after the timed region)")
    ap.add_argument("--graph", action="store_true", help="replay the step from a HIP graph (models.GraphedForward) instead of issuing it eagerly")
    ap.add_argument("--exec", dest="exec_mode", choices=["auto", "eager", "graph"], default="auto",
                    help="inference: how the step is issued.  Same kernels, same results; eager issue costs the host ~1.3-1.5 ms per forward "
                         "(Python + ctypes per launch), a HIP-graph replay none but the runtime orders parallel branches its own way. "
                         "auto = time a few steps of both during warm-up and keep the faster")
    args = ap.parse_args()
    if args.parity_trained > 0 and not args.full:
        ap.error("--parity-trained is part of the parity block: add --full")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` with no launcher: start N ranks of this same command under torch.distributed.run (one process per GPU,
        # RCCL over xGMI; 127.0.0.1 rendezvous -- the container hostname may not resolve) and hand their exit code on.  Rank 0 of
        # the child job prints the ONE JSON line.
        raise SystemExit(self_launch(args.gpus))

    import hesic_amd
    from hesic_amd import functional as Fn, geometry, models, synthetic
    from hesic_amd.train import init_distributed
    import torch.distributed as dist
    if args.warp_align_corners is not None:
        geometry.DEFAULT_ALIGN_CORNERS = bool(args.warp_align_corners)
    if args.analysis is not None:
        Fn.set_analysis_precision(args.analysis)
    if args.sweep and not (args.height or args.width):
        args.height, args.width = 860, 1080

    rank, world, local = init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if args.dtype is None:
        args.dtype = "bf16" if args.mode == "train" else "f16"
    if args.mode == "train" and args.dtype == "f16":
        raise SystemExit("--mode train runs in bf16 (or f32): gradients need the fp32 exponent range")
    cdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]
    hesic_amd.set_compute_dtype(cdt)

    net = (models.HSIC if args.model == "hsic" else models.HSICJoint)()
    synthetic.fill_state_dict_(net.state_dict())
    P_cpu = {k: v.clone() for k, v in net.state_dict().items()} if rank == 0 else None
    net = net.to(dev).eval()

    # synthetic pairs: rank r gets pairs [r*B, (r+1)*B); one generated pair set is tiled if B is large
    uniq = min(args.batch, 8)          # round 6: every pair of the timed C2 batch is a distinct pair (rounds 1-5 tiled four)
    H_img, W_img = args.height or args.size, args.width or args.size
    x1, x2, Hm = synthetic.stereo_batch(rank * uniq, uniq, H_img, W_img)
    reps = -(-args.batch // uniq)
    x1, x2, Hm = (t.repeat(reps, *([1] * (t.dim() - 1)))[:args.batch].to(dev) for t in (x1, x2, Hm))
    x1p, x2p = models.pad_to_multiple(x1), models.pad_to_multiple(x2)      # no-op at 512x512

    if args.mode == "train":
        return train_main(args, net, P_cpu, (x1p, x2p, Hm), rank, world, dev, H_img, W_img)
    if args.sweep:
        return sweep_main(args, (x1, x2, x1p, x2p, Hm), rank, world, dev, H_img, W_img)

    # the timed loop rotates over NBUF different resident batches (same shapes, different pairs): no step re-reads the inputs
    # the previous one left in the Infinity Cache
    NBUF = 4
    pool = [(x1, x2, x1p, x2p, Hm)]
    for j in range(1, NBUF):
        a, b, h = synthetic.stereo_batch((world * j + rank) * uniq, uniq, H_img, W_img)
        a, b, h = (t.repeat(reps, *([1] * (t.dim() - 1)))[:args.batch].to(dev) for t in (a, b, h))
        pool.append((a, b, models.pad_to_multiple(a), models.pad_to_multiple(b), h))

    # bits / squared error of a batch are reduced on a stream of their own: the six small-grid reductions (and the joins in
    # front of them) then run beside the first kernels of the NEXT batch instead of holding the main stream for ~100 us
    # (no fifth stream: the schedule's streams fill the runtime's four hardware queues; the stream view 1's rate branch uses is idle
    # from the middle of a forward to ~0.3 ms into the next one)
    mstream = models.metrics_stream(dev)

    def metrics_async(out, a, b):
        mstream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(mstream), torch.no_grad():
            models.hand_over((out["x1_hat"], out["x2_hat"], *out["likelihoods"].values()), mstream)
            return models.rate_distortion(out, a, b)

    def step(i=0):
        a, b, ap_, bp_, h = pool[i % NBUF]
        with torch.no_grad():
            out = net(ap_, bp_, h)
        return out, metrics_async(out, a, b)

    eager_step = step
    exec_mode = "graph" if args.graph else args.exec_mode
    picked = {"mode": exec_mode}
    if exec_mode in ("graph", "auto"):
        graphed = models.GraphedForward(net, x1p, x2p, Hm, with_metrics=False)

        def graph_step(i=0):  # same work: graph replay of the forward (inputs copied into its static buffers), then the reductions
            a, b, ap_, bp_, h = pool[i % NBUF]
            torch.cuda.current_stream().wait_stream(mstream)      # the replay overwrites the static outputs the last reductions read
            out, _ = graphed(ap_, bp_, h)
            return out, metrics_async(out, a, b)

        if exec_mode == "auto":
            def trial(fn, n=40):
                for i in range(15):          # the eager path needs ~10 steps until the side streams' allocator pools have settled
                    fn(i)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for i in range(n):
                    fn(i)
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / n
            te, tg = trial(eager_step), trial(graph_step)
            if world > 1:           # one decision for the job: the slowest rank's view of each mode
                t = torch.tensor([te, tg], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                te, tg = float(t[0]), float(t[1])
            picked = {"mode": "graph" if tg < te else "eager", "auto": {"eager_ms": round(te * 1e3, 3), "graph_ms": round(tg * 1e3, 3)}}
        if picked["mode"] == "graph":
            step = graph_step
    for i in range(args.warmup):
        out, rd = step(i)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out, rd = step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed, ranks_info = job_time(elapsed, world, dev, args.batch * args.steps)
    if rank == 0 and args.dump_outputs and args.steps > 0:
        dump_outputs(args.dump_outputs, flat_outputs(out, rd))          # before anything else runs: a graph replay overwrites `out`
    m_gpu = models.metrics_from(rd)

    # roofline of the dominant kernel, measured live with HIP events on the launch stream
    roof, s = None, None
    from hesic_amd import _lib as L_
    if args.full:
        overlap, models.OVERLAP_STREAMS = models.OVERLAP_STREAMS, False     # one stream: an event pair brackets ONE kernel
        with KernelMeter(L_) as km:
            for _ in range(3):
                eager_step()
            s = km.summary()
        models.OVERLAP_STREAMS = overlap
    if s:
        peak = MFMA_BF16_PEAK_TFLOPS if args.dtype != "f32" else MFMA_F32_PEAK_TFLOPS
        traffic, traffic_src = None, None     # HBM-side bytes per launch from the committed rocprofv3 PMC passes (profiles/make_pmc_json.py)
        pj = os.path.join(ROOT, "profiles", "pmc_igemm.json")
        if os.path.exists(pj):
            try:
                key = f"{args.model}_{args.dtype}_b{args.batch}_{args.size}"
                pmc = json.load(open(pj))
                traffic = pmc.get(key, {}).get("per_kernel", {}).get(s["kernel"], {}).get("hbm_bytes_per_launch")
                if traffic is not None:       # NOT measured by this run: rocprofv3 --pmc passes of an earlier commit, kept under profiles/
                    traffic_src = {"file": "profiles/pmc_igemm.json", "commit": pmc.get("_commit"), "collected": pmc.get("_collected"),
                                   "note": "HBM bytes per launch from separate rocprofv3 --pmc passes (profiles/make_pmc_json.py), not from this run"}
            except Exception:
                traffic = None
        roof = {"kernel": s["kernel"], "bound": "mfma",
                "achieved": round(s["tflops"], 2), "peak": peak, "unit": "TFLOP/s", "frac": round(s["tflops"] / peak, 4),
                "traffic": traffic, "traffic_source": traffic_src,
                "mfma_products_per_mac": s["mfma_products_per_mac"], "executed_tflops": round(s["executed_tflops"], 2),
                "executed_frac": round(s["executed_tflops"] / peak, 4),
                "flop_convention": "achieved / frac: algorithmic 2 x MAC of the layer (SURVEY 8d) per launch over its HIP-event time; executed_*: the bf16 MFMA "
                                   "work the launch performs -- 3 products per MAC for the hi/lo (bf16x3) analysis launches, equal to achieved otherwise", "launches_per_step": s["launches"] // 3, "avg_launch_us": round(s["avg_us"], 2),
                "gflop_per_launch": round(s["flops_per_launch"] / 1e9, 3), "other_conv_kernels": s["all"],
                # the HBM-bound kernels of the path against the 8 TB/s peak (north_star: "achieved HBM GB/s for the warp")
                "streaming_kernels": km.streaming}
        # the warp alone, 20 launches back to back between ONE pair of HIP events: the single-launch bracket above carries ~4 us of launch
        # latency on a ~12 us kernel (profiles/scripts/warp_time.py: 11.7 us from a graph)
        try:
            wk = next((k for k in km.streaming if k.startswith("warp_perspective")), None)
            if wk is not None:
                from hesic_amd import functional as Fn_
                hw = x1.shape[-2:]
                for _ in range(3):
                    Fn_.warp_perspective(x1, Hm, tuple(hw))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    Fn_.warp_perspective(x1, Hm, tuple(hw))
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / 20
                by = km.streaming[wk]["bytes_per_launch"]
                km.streaming[wk]["back_to_back"] = {"launches": 20, "avg_launch_us": round(us, 2), "achieved": round(by / us / 1e3, 1), "frac": round(by / us / 1e3 / HBM_PEAK_GBS, 4),
                                                    "note": "the SAME 25 MB source and destination 20 times between one event pair: they stay in the 256 MB Infinity Cache, so this is "
                                                            "cache-assisted bandwidth (the kernel without its launch latency), not HBM bandwidth; the single-launch figure above is the "
                                                            "roofline entry (ADVICE r5)"}
        except Exception as e:                     # a report line, never the reason a bench run fails
            print(f"# warp back-to-back timing skipped: {e}", file=sys.stderr)
        if rank == 0 and world == 1 and args.dtype != "f32" and not args.no_power_state:
            try:
                _i = [0]

                def _one():
                    _i[0] += 1
                    step(_i[0])
                roof["power_state"] = power_state(_one, args.dtype, dev)
                pl = roof["power_state"].get("mfma_loop_random_operands", {}).get("tflops")
                if pl:
                    roof["executed_frac_of_mfma_loop_at_power_cap"] = round(s["executed_tflops"] / pl, 4)
            except Exception as e:
                print(f"# power_state skipped: {e}", file=sys.stderr)

    if rank == 0:
        pairs = world * args.batch * args.steps
        res = {
            "metric": "stereo-pairs/sec encode+decode @512x512; bpp & PSNR delta vs reference",
            "value": round(pairs / elapsed, 2), "unit": "stereo-pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "full": args.full,
            "config": {"workload": f"{'HESIC' if args.model == 'hsic' else 'HESIC+'} eval forward (encode+decode) + bpp/PSNR, "
                                   f"{H_img}x{W_img} stereo pairs, batch {args.batch}/GPU, random-init-shaped deterministic weights",
                       "pairs_per_step": world * args.batch, "sharding": f"pairs over {world} GPU(s), no collective on the path",
                       "analysis": (Fn.analysis_precision() if args.dtype != "f32" else "fp32"),
                       "warp_align_corners": bool(geometry.DEFAULT_ALIGN_CORNERS), "issue": picked},
            "model_tflops": round(pairs * gflop_per_pair(args.model, x1p.shape[-2], x1p.shape[-1]) / elapsed / 1e3, 2),
            "roofline": roof,
            "gpu_metrics_last_batch": {"bpp": round(m_gpu["bpp"], 5), "psnr": round(m_gpu["psnr"], 4)},
        }
        if ranks_info is not None:
            res["ranks"] = ranks_info
        if args.full and world == 1 and not args.no_cpu_baseline:
            square = not (args.height or args.width)
            npar = min(8, args.batch) if square else 1          # every distinct pair of the timed batch
            base, m_cpu = cpu_baseline(args.model, P_cpu, args.size if square else 512, parity_pairs=npar)
            res["cpu_baseline"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in base.items()}
            per_pair = []
            for j, mc in enumerate([m_cpu] + m_cpu["more"]):
                with torch.no_grad():
                    xa, xb, hh = (t.to(dev) for t in synthetic.stereo_batch(j, 1, 512, 512)) if not square else (x1[j:j + 1], x2[j:j + 1], Hm[j:j + 1])
                    oj = net(xa, xb, hh)
                    mj = models.metrics_from(models.rate_distortion(oj, xa, xb))
                fl = {k: float((oj[k].float().cpu().to(torch.int16) != v).float().mean()) for k, v in mc["y_hat"].items()}
                per_pair.append({"dbpp": mj["bpp"] - mc["bpp"], "dpsnr": mj["psnr"] - mc["psnr"], "flips": fl, "bpp": mc["bpp"], "psnr": mc["psnr"]})
            # the set average is what the reference's evaluation reports (test3real.py:110-122: bpp and PSNR averaged over the pairs);
            # pair 0 alone (the figure of rounds 1-3 so far) and the worst pair stand next to it
            dbpp = abs(sum(q["dbpp"] for q in per_pair) / len(per_pair))
            dpsnr = abs(sum(q["dpsnr"] for q in per_pair) / len(per_pair))
            bpp_o = sum(q["bpp"] for q in per_pair) / len(per_pair)
            flips = {k: max(q["flips"][k] for q in per_pair) for k in per_pair[0]["flips"]}
            cond_flips, dms = None, None
            if "ms_ssim" in m_cpu and square:
                with torch.no_grad():
                    o0 = net(x1[:1], x2[:1], Hm[:1])
                    ms_gpu = float((models.ms_ssim(o0["x1_hat"], x1[:1])[0] + models.ms_ssim(o0["x2_hat"], x2[:1])[0]) / 2)
                dms = {"gpu": round(ms_gpu, 7), "oracle": round(m_cpu["ms_ssim"], 7), "abs_diff": float("%.3g" % abs(ms_gpu - m_cpu["ms_ssim"]))}
            if "y1_hat_w" in m_cpu and square and geometry.DEFAULT_ALIGN_CORNERS:
                with torch.no_grad():
                    o0 = net(x1[:1], x2[:1], Hm[:1])
                    yw = net.encoder1.latent(geometry.warp_perspective(o0["x1_hat"], Hm[:1], tuple(x1.shape[-2:])), want_lo=False)[1]
                cond_flips = round(float((torch.round(yw.float()).cpu().to(torch.int16) != m_cpu["y1_hat_w"]).float().mean()), 6)
            worst_dbpp, worst_dpsnr = max(abs(q["dbpp"]) for q in per_pair), max(abs(q["dpsnr"]) for q in per_pair)
            res["parity"] = {"abs_dbpp": round(dbpp, 6), "rel_dbpp": round(dbpp / bpp_o, 6), "abs_dpsnr_db": round(dpsnr, 6),
                             "pairs": len(per_pair),
                             "pair0": {"abs_dbpp": round(abs(per_pair[0]["dbpp"]), 6), "abs_dpsnr_db": round(abs(per_pair[0]["dpsnr"]), 6)},
                             "worst_pair": {"abs_dbpp": round(worst_dbpp, 6), "abs_dpsnr_db": round(worst_dpsnr, 6)},
                             "per_pair_dbpp": [round(q["dbpp"], 6) for q in per_pair], "per_pair_dpsnr_db": [round(q["dpsnr"], 6) for q in per_pair],
                             "bpp_oracle": round(bpp_o, 5), "psnr_oracle": round(sum(q["psnr"] for q in per_pair) / len(per_pair), 4),
                             "latent_flips": {k: round(v, 6) for k, v in flips.items()},
                             "conditioning_latent_flips_y1_hat_w": cond_flips,
                             "ms_ssim_pair0": dms,
                             "bars": {"latent_flips": 1e-3, "abs_dpsnr_db": 1e-3, "abs_dbpp": 1e-3, "rel_dbpp": 1e-3},
                             "met": {"latent_flips": bool(max(flips.values()) <= 1e-3), "abs_dpsnr_db": bool(dpsnr < 1e-3),
                                     "abs_dbpp": bool(dbpp < 1e-3), "rel_dbpp": bool(dbpp < 1e-3 * bpp_o),
                                     "abs_dbpp_every_pair": bool(worst_dbpp < 1e-3), "abs_dpsnr_db_every_pair": bool(worst_dpsnr < 1e-3)},
                             "analysis": Fn.analysis_precision() if args.dtype != "f32" else "fp32",
                             "latents": "fp32 (y, z, sigma, mu from the fp32 accumulators)" if (args.dtype == "f32" or Fn.FP32_LATENTS) else "bf16",
                             "note": f"{args.dtype} GPU path vs fp32 CPU oracle on the {len(per_pair)} distinct pair(s) of the timed workload, random-init-shaped "
                                     "weights (bpp ~5.5: the absolute bpp bar is 1.8e-4 RELATIVE here).  abs_* = |mean over the pairs| (the reference "
                                     "reports set averages), latent_flips = the worst pair; pair0 / worst_pair / per_pair_* give every pair; "
                                     "conditioning_latent_flips_y1_hat_w = pair 0's round(encoder1(warp(x1_hat))) (not transmitted: it conditions view 2's "
                                     "entropy parameters; single 16-bit operands, no bar of its own -- its effect is inside dbpp); "
                                     "--parity-trained adds trained operating points"}
            if args.parity_trained > 0:
                res["parity"]["trained"] = trained_parity(args.model, args.parity_trained, args.parity_train_steps, 512, lmbda=args.lmbda,
                                                          log=lambda t: print(t, file=sys.stderr, flush=True))
        else:
            res["cpu_baseline"] = None
        default_workload = args.model == "hsic" and args.batch == 8 and not (args.height or args.width) and args.size == 512
        if args.full and world == 1 and default_workload and not args.no_secondary:
            res["secondary"] = secondary_block(dev, lmbda=args.lmbda)
            # round 5: the other modes of C2 with their parity, the C5 sweep, path A and the training step with RCCL in the graph (~15 s)
            if not args.no_cpu_baseline and args.dtype != "f32":
                res["secondary"]["c2_other_modes"] = secondary_modes(dev, [m_cpu] + m_cpu["more"])
            res["secondary"].update(secondary_sweep_and_path_a(dev, oracle_pairs=None if args.no_cpu_baseline or args.dtype == "f32" else [m_cpu] + m_cpu["more"]))
            res["secondary"]["hesic_en_b8"] = secondary_hesic_en(dev)
            res["secondary"]["train_step_hesic_b8_rccl_1rank"] = secondary_train_rccl(dev, lmbda=args.lmbda)
        emit_line(res)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
