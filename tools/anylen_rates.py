#!/usr/bin/env python3
"""Rates of the any-length path (include/rtlws_anylen.h, Bluestein over the four-step transform) for cmplx_u8
frames, K = 1, f64 rows -- in one process, device events, three alternating rounds, outputs compared first:

  against the direct sum    N = 1000, 5000, 8000 through the plan and through rtlws_spectra_batch_f64 (today's
                            path for lengths that are no power of two) on the same frames
  against rtlws_long.h      N = 12000, 100000, 500000 through the plan, beside rtlws_long.h at the same M = 2^15,
                            2^18, 2^20 on the same number of frames.  A Bluestein frame is two M-point transforms and
                            a pointwise product: about 112 M bytes against the long run's 34 M, 3.3 x.
  against the CPU (--cpu)   the oracle on 16 threads.  Its transform of a length that is no power of two is a direct
                            long-double sum, O(N^2): it is timed up to N = 12000 and not above (hours per frame).

    python tools/anylen_rates.py [--cpu] > profiles/anylen_rates.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from long_frames_rates import time_launches

SHORT = ((1000, 2048), (5000, 1024), (8000, 1024))            # (N, frames): one workgroup per frame in the direct sum
LONG = (12000, 100000, 500000)
LONG_POINTS = 1 << 24                                         # M * frames: 512 MiB of workspaces
ROUNDS, STEPS = 3, 4
TOL = 1e-10                                                   # the strict metric (tests/helpers.py)


def strict_err(got, ref):
    floor = 1e-9 * np.abs(ref).max(axis=-1, keepdims=True)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), floor)).max())


def main(with_cpu):
    import torch
    import rtlws
    import anylen_ref
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    L = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cfg, plans, notes = [], [], []

    def frames_of(N, F):
        return torch.randint(0, 256, (F, N, 2), dtype=torch.uint8, device=dev, generator=gen)

    for N, F in SHORT:
        src, out_a, out_d = frames_of(N, F), torch.zeros((F, N), dtype=torch.float64, device=dev), torch.zeros((F, N), dtype=torch.float64, device=dev)
        desc = rtlws.make_desc(N)
        plan = rtlws.AnyLenPlan(eng, desc, F)
        plans.append(plan)
        run_a = lambda i, p=plan, s=src, o=out_a, f=F: p.run(s.data_ptr(), f, o.data_ptr(), stream=stream)
        run_d = lambda i, d=desc, s=src, o=out_d, f=F: eng.spectra_batch_f64(d, s.data_ptr(), f, o.data_ptr(), stream=stream)
        run_a(0)
        run_d(0)
        torch.cuda.synchronize()
        a, d = out_a.cpu().numpy(), out_d.cpu().numpy()
        ref = anylen_ref.rows(src[:8].cpu().numpy(), N, 1)
        notes.append("N=%d: plan against the direct sum %.3g, plan against np.fft %.3g, direct sum against np.fft %.3g"
                     % (N, strict_err(a, d), strict_err(a[:8], ref), strict_err(d[:8], ref)))
        assert strict_err(a, d) <= TOL and strict_err(a[:8], ref) <= TOL
        cfg.append(("anylen N=%d (M=2^14)" % N, N, F, run_a))
        cfg.append(("direct sum N=%d" % N, N, F, run_d))
    for N in LONG:
        m = rtlws.anylen_conv_log2(rtlws.make_desc(N))
        M, F = 1 << m, LONG_POINTS >> m
        src, out = frames_of(M, F), torch.zeros((F, M), dtype=torch.float64, device=dev)     # the first F * N samples serve the plan
        plan = rtlws.AnyLenPlan(eng, rtlws.make_desc(N), F)
        lplan = rtlws.LongPlan(eng, rtlws.make_desc(M), F)
        plans += [plan, lplan]
        assert plan.workspace_bytes == 32 * LONG_POINTS and lplan.workspace_bytes == 16 * LONG_POINTS    # one group each
        run_a = lambda i, p=plan, s=src, o=out, f=F: p.run(s.data_ptr(), f, o.data_ptr(), stream=stream)
        run_l = lambda i, p=lplan, s=src, o=out, f=F: p.run(s.data_ptr(), f, o.data_ptr(), stream=stream)
        run_a(0)
        torch.cuda.synchronize()
        a = out.reshape(-1)[:2 * N].reshape(2, N).cpu().numpy()
        ref = anylen_ref.rows(src.reshape(-1, 2)[:2 * N].cpu().numpy(), N, 1)
        notes.append("N=%d: plan against np.fft %.3g" % (N, strict_err(a, ref)))
        assert strict_err(a, ref) <= TOL
        cfg.append(("anylen N=%d (M=2^%d)" % (N, m), N, F, run_a))
        cfg.append(("long N=2^%d" % m, M, F, run_l))

    for _, _, _, launch in cfg:                                  # warm up every shape
        launch(0)
    torch.cuda.synchronize()
    secs = {label: [] for label, _, _, _ in cfg}
    for _ in range(ROUNDS):                                      # alternating: every configuration once per round
        for label, _, _, launch in cfg:
            secs[label].append(time_launches(L, eng, stream, launch, STEPS))
    print("# cmplx_u8, K = 1, f64 rows; device events over %d launches, %d alternating rounds (median; min-max)" % (STEPS, ROUNDS))
    print("# outputs first, strict metric (bound %.0e):" % TOL)
    for n in notes:
        print("#   " + n)
    print("# %-28s %7s %10s %12s %12s %s" % ("configuration", "frames", "ms/launch", "spectra/s", "points/s", "spread ms"))
    med = {}
    for label, N, F, _ in cfg:
        s = sorted(secs[label])
        med[label] = t = s[len(s) // 2]
        print("  %-28s %7d %10.3f %12.4g %12.4g %.3f-%.3f" % (label, F, 1e3 * t, F / t, F * N / t, 1e3 * s[0], 1e3 * s[-1]))
    print("# per frame: the plan against the direct sum (> 1: the plan is faster), the plan against rtlws_long.h at the same M"
          " (expected by bytes: about 3.3 x the long run's time)")
    labels = [c[0] for c in cfg]
    for a, b in zip(labels[0::2], labels[1::2]):
        sa, sb = secs[a], secs[b]
        r = [y / x for x, y in zip(sa, sb)] if b.startswith("direct") else [x / y for x, y in zip(sa, sb)]
        what = "direct sum / plan" if b.startswith("direct") else "plan / long"
        print("  %-28s %-18s %.2fx (rounds %.2f-%.2f)" % (a, what, sorted(r)[len(r) // 2], min(r), max(r)))
    if with_cpu:
        from oracle import pyoracle as po
        print("# the oracle on 16 CPU threads (f64 result from a direct long-double sum at these lengths), 16 frames, one call")
        for N in (1000, 5000, 8000, 12000):
            iq = np.random.default_rng(N).integers(0, 256, size=(16, N, 2), dtype=np.uint8)
            outb = np.empty((16, N))
            t0 = time.perf_counter()
            po.batch_spectra_u8(iq, N, nthreads=16, out=outb)
            t = time.perf_counter() - t0
            gpu = [c for c in cfg if c[0].startswith("anylen N=%d " % N)][0]
            print("  oracle N=%d: %.4g spectra/s; the plan: %.4g spectra/s, %.3gx" % (N, 16 / t, gpu[2] / med[gpu[0]], gpu[2] / med[gpu[0]] / (16 / t)))
        print("  oracle N=100000, 500000: not measured (O(N^2): hours per frame)")
    for p in plans:
        p.close()
    eng.close()


if __name__ == "__main__":
    main("--cpu" in sys.argv)
