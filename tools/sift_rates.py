#!/usr/bin/env python3
"""Sift of single-pulse peaks on device-resident arrays: the three launches of rtlws_sift_run (include/rtlws_sift.h) per
shape against the device-to-host copy of the same three arrays in the same process, which is what any sift on the host
pays before it starts.

    python tools/sift_rates.py [--out FILE]      1024 and 4096 trials x 16 widths x 1024 segments, rt 16, rs 2, a
                                                 threshold that about 1e-4 of the events pass; device events, one
                                                 process, three alternating rounds

The method is tools/pulse_rates.py's: every round times `steps` runs between two events; consecutive runs read different
arrays (two sets of peak, at and mom) and write different lists.  The arrays are made on the device: every segment its own
mean and deviation, the peaks of every width the noise's, so that a width's score is about normal and the best of 16 a
little above; the threshold is the (1 - 1e-4) quantile of the scores of the first run.  Per shape: microseconds per run of
the three launches together, min .. max of the rounds; the bytes 8 K T S + 16 T S read once over that time as a fraction of
8 TB/s (the run itself reads the places of its candidates alone, 4 K T S + 16 T S and the 8 T S of its plane twice); the
same for the copy of peak, at and mom into pinned host memory; and whether the rounds' ranges overlap.  The lines go to
FILE (default profiles/sift_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)
SEG, RT, RS, PASS, MAX_CAND, STEPS = 1024, 16, 2, 1e-4, 1 << 16, 20


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "sift_rates.txt")
    if args and args[0] == "--out":
        out_path = args[1]

    import torch
    import rtlws
    import rtlws.sift
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("peak, at and mom on the device as rtlws_pulse_run lays them out; rtlws_sift_run (three launches) against the copy of the three "
        "arrays to pinned host memory in one process; device events, %d runs a round, three alternating rounds, two sets of arrays in "
        "turn; HBM peak taken as %.0f TB/s" % (STEPS, HBM_PEAK / 1e12))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fns, steps):
        times = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                fn(0), fn(1)
                e0.record()
                for i in range(steps[name]):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / steps[name])
        return times

    K = len(WIDTHS)
    w = torch.tensor(WIDTHS, dtype=torch.float64, device=dev)
    for T in (1024, 4096):
        S, nout = 1024, 1024 * SEG
        rc, blocks, threads, lds, tile_t, tile_s, nseg = rtlws.sift.geometry(WIDTHS, SEG, RT, RS, T, nout)
        assert rc == 0 and nseg == S
        plan = rtlws.sift.SiftPlan(eng, WIDTHS, SEG, RT, RS)
        peaks, ats, moms = [], [], []
        for seed in (1, 2):
            g = torch.Generator(device=dev).manual_seed(seed)
            mu = 1.0 + 4.0 * torch.rand((T, 1, S), dtype=torch.float64, device=dev, generator=g)
            sd = 0.5 + 1.5 * torch.rand((T, 1, S), dtype=torch.float64, device=dev, generator=g)
            z = torch.randn((T, K, S), dtype=torch.float32, device=dev, generator=g)
            peaks.append((w[None, :, None] * mu + z.double() * w.sqrt()[None, :, None] * sd).float().contiguous())
            ats.append(torch.randint(0, SEG, (T, K, S), dtype=torch.int32, device=dev, generator=g) + (torch.arange(S, dtype=torch.int32, device=dev) * SEG)[None, None, :])
            moms.append(torch.stack([SEG * mu[:, 0], SEG * (sd[:, 0] ** 2 + mu[:, 0] ** 2)], dim=2).contiguous())
            del mu, sd, z
        work = torch.empty(plan.work_bytes(T, nout) // 4, dtype=torch.int32, device=dev)
        cands = [torch.zeros(MAX_CAND * 8, dtype=torch.int32, device=dev) for _ in range(2)]
        counts = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(2)]
        score = torch.empty(T * S, dtype=torch.float32, device=dev)
        host = [torch.empty(a.shape, dtype=a.dtype, pin_memory=True) for a in (peaks[0], ats[0], moms[0])]

        def run(i, thr, plane=None):
            plan.run(peaks[i % 2].data_ptr(), ats[i % 2].data_ptr(), moms[i % 2].data_ptr(), T, nout, thr, MAX_CAND, work.data_ptr(), cands[i % 2].data_ptr(),
                     counts[i % 2].data_ptr(), plane, None, stream=stream)

        run(0, float("inf"), score.data_ptr())
        torch.cuda.synchronize()
        thr = float(torch.sort(score).values[int((1.0 - PASS) * T * S)])
        del score

        def copy(i):
            for h, d in zip(host, (peaks[i % 2], ats[i % 2], moms[i % 2])):
                h.copy_(d, non_blocking=True)

        times = timed({"sift": lambda i: run(i, thr), "copy": copy}, {"sift": STEPS, "copy": 3})
        torch.cuda.synchronize()
        found = [c.cpu().numpy().tolist() for c in counts]
        ts, tc = times["sift"], times["copy"]
        nominal, read = 8 * K * T * S + 16 * T * S, 4 * K * T * S + 16 * T * S + 16 * T * S
        say("%d trials x %d widths x %d segments, rt %d, rs %d, threshold %.3f: %s candidates of %s events at or above it (%.2e of %d); workgroups %s, LDS %s B"
            % (T, K, S, RT, RS, thr, "/".join(str(f[0]) for f in found), "/".join(str(f[1]) for f in found), found[0][1] / (T * S), T * S, blocks, lds))
        say("    rtlws_sift_run    %9.1f .. %9.1f us/run   8KTS + 16TS = %.1f MB over it: %.3f .. %.3f of the HBM peak; the %.1f MB it reads and writes: %.3f .. %.3f  (%s)"
            % (min(ts), max(ts), nominal / 1e6, nominal / max(ts) * 1e6 / HBM_PEAK, nominal / min(ts) * 1e6 / HBM_PEAK, read / 1e6, read / max(ts) * 1e6 / HBM_PEAK,
               read / min(ts) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in ts)))
        say("    copy to the host  %9.1f .. %9.1f us       = %.1f times the run's median; %.1f GB/s; the ranges %s  (%s)"
            % (min(tc), max(tc), float(np.median(tc)) / float(np.median(ts)), nominal / float(np.median(tc)) / 1e3, "do not overlap" if min(tc) > max(ts) else "OVERLAP",
               " ".join("%.1f" % x for x in tc)))
        plan.close()
        del peaks, ats, moms, work, cands, counts, host

    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
