#!/usr/bin/env python3
"""Cleaning of a device-resident waterfall (include/rtlws_clean.h): the time of the three launches of rtlws_clean_run at
1024 channels x 65 536 rows and 4096 x 16 384, each in blocks of 1024 and of 8192 rows, with thresholds of 6 MADs and the
zero-DM filter; and, to tell the stages apart from outside, the same run with no thresholds (stage 2 sorts nothing) and
with the filter off (stage 3 has no tree and no division).

    python tools/clean_bench.py [--out FILE]    device events around the launches only, one process, three alternating
                                                rounds; the lines go to FILE (default profiles/clean.txt) and to stdout
    python tools/clean_bench.py --once          every shape three times and nothing timed: what a kernel trace is taken of

The floor is two reads and one write of the waterfall, 12 nchan nrows bytes, at the HBM peak, which is taken, not
measured, as 8.0 TB/s (the guide's chip table).  Both waterfalls are 268 MB, more than the 256 MiB Infinity Cache, and
two sets of inputs and outputs are used in turn."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
SHAPES = ((1024, 65536, 1024), (1024, 65536, 8192), (4096, 16384, 1024), (4096, 16384, 8192))      # nchan, nrows, block_rows
INF = float("inf")


def main():
    args = sys.argv[1:]
    once = "--once" in args
    out_path = os.path.join(ROOT, "profiles", "clean.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]

    import torch
    import rtlws
    import rtlws.clean as clean
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns, steps):
        times = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                fn(0), fn(1)
                H.rtlws_event_record(e0, eng.h, stream)
                for i in range(steps):
                    fn(i)
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / steps)
        return times

    say("f32 rows on the device; device events around the three launches only, three alternating rounds of 20 runs, two sets of inputs "
        "and of outputs in turn; the HBM peak taken, not measured, as %.1f TB/s" % (HBM_PEAK / 1e12))
    for nchan, nrows, B in SHAPES:
        rows = [torch.rand((nrows, nchan), dtype=torch.float32, device=dev) * (1.0 + 0.2 * torch.sin(torch.arange(nchan, device=dev) / 7.0)) for _ in range(2)]
        outs = [torch.empty((nrows, nchan), dtype=torch.float32, device=dev) for _ in range(2)]
        nb = -(-nrows // B)
        keep = torch.empty((nb, nchan), dtype=torch.uint8, device=dev)
        plans = {"6 MADs, zero-DM": clean.CleanPlan(eng, nchan, B, None, 6.0, 6.0, True),
                 "no thresholds, zero-DM": clean.CleanPlan(eng, nchan, B, None, INF, INF, True),
                 "6 MADs, no zero-DM": clean.CleanPlan(eng, nchan, B, None, 6.0, 6.0, False)}
        fns = {name: (lambda i, p=p: p.run(rows[i % 2].data_ptr(), nchan, nrows, outs[i % 2].data_ptr(), nchan, keep.data_ptr(), stream=stream))
               for name, p in plans.items()}
        rc, blocks, threads, lds, nblocks, work, _ = clean.geometry(nchan, B, nrows)
        assert rc == 0
        if once:
            for fn in fns.values():
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
        else:
            times = timed(fns, 20)
            floor = 12.0 * nchan * nrows / HBM_PEAK * 1e6
            say("%d channels x %d rows in blocks of %d (%d blocks): workgroups %s of %s threads, LDS %s B, workspace %.2f MB; floor %.1f us"
                % (nchan, nrows, B, nblocks, blocks, threads, lds, work / 1e6, floor))
            for name, t in times.items():
                say("    %-24s %8.1f .. %8.1f us/run = %.3f .. %.3f of the floor's rate  (%s)"
                    % (name, min(t), max(t), floor / max(t), floor / min(t), " ".join("%.1f" % x for x in t)))
            kept = int(keep.sum().item())
            say("    kept %d of %d (block, channel) pairs" % (kept, nb * nchan))
        for p in plans.values():
            p.close()
        del rows, outs
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    if not once:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
