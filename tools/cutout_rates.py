#!/usr/bin/env python3
"""Cutouts of single-pulse candidates on device-resident arrays: the two launches of rtlws_cutout_run
(include/rtlws_cutout.h) over 64 and over 1024 candidates of a 1024-channel waterfall against the device-to-host copy of the
same rows and series in the same process, which is what a caller without this library pays before it can draw a plane.

    python tools/cutout_rates.py [--out FILE]    1024 channels x 262144 rows, 256 trials of a dispersion sweep, nx 64,
                                                 nf 64, bin 4, rq 16, dq 1; device events, one process, three
                                                 alternating rounds

The method is tools/sift_rates.py's: every round times `steps` runs between two events; consecutive runs read different
lists (eight of them, the candidates at random trials and places, so that no run finds its rows in a cache the run before
filled) and write different planes.  Per count of candidates: microseconds per run of the two launches together and of each
launch alone, min .. max of the rounds; the bytes nx b nchan 4 per candidate, the rows of the band-time plane read once,
over the band-time launch's time as a fraction of 8 TB/s; that launch again with every candidate moved to trials
16 .. 23, whose sweeps are shallow, so that what the sweep costs shows; the copy, per candidate, of the rows n0 .. n0 + nx b - 1 + the
trial's largest delay (whole rows: they are contiguous) and of the 2 rq + 1 windows of the series into pinned host memory;
and whether the rounds' ranges overlap.  The lines go to FILE (default profiles/cutout_rates.txt) and to stdout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
NCHAN, NSAMP, NTRIALS, NX, NF, BIN, RQ, DQ, WIDTH = 1024, 262144, 256, 64, 64, 4, 16, 1, 4
NSETS, STEPS = 8, 20


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cutout_rates.txt")
    if args and args[0] == "--out":
        out_path = args[1]

    import torch
    import rtlws
    import rtlws.cutout
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    delays = rtlws.dedisp_delays(NCHAN, 1, 1400e6, 300e6, 64e-6, NTRIALS, 0.0, 2.0)
    most = int(delays.max())
    say("%d channels x %d rows (sweep of up to %d rows), %d trials; nx %d, nf %d, bin %d, rq %d, dq %d; rtlws_cutout_run (two launches) against "
        "the copy of every candidate's rows and series windows to pinned host memory in one process; device events, %d runs of 1024 candidates a round "
        "(16 times as many of 64), three alternating rounds, %d lists in turn; HBM peak taken as %.0f TB/s"
        % (NCHAN, NSAMP, most, NTRIALS, NX, NF, BIN, RQ, DQ, STEPS, NSETS, HBM_PEAK / 1e12))
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randn((NSAMP + most, NCHAN), dtype=torch.float32, device=dev, generator=g)
    series = torch.randn((NTRIALS, NSAMP), dtype=torch.float32, device=dev, generator=g)
    plan = rtlws.cutout.CutoutPlan(eng, delays, None, [WIDTH], [BIN], NX, NF, RQ, DQ)
    ndm = 2 * RQ + 1
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

    for ncand in (64, 1024):
        rng = np.random.default_rng(ncand)
        steps = STEPS * 1024 // ncand                             # as many candidates a round either way
        hosts_lists, lists = [], []
        for _ in range(NSETS):
            cand = np.zeros((ncand, 8), np.int32)
            cand[:, 0] = rng.integers(RQ * DQ, NTRIALS - RQ * DQ, ncand)
            cand[:, 3] = rng.integers(NX * BIN, NSAMP - NX * BIN, ncand)
            hosts_lists.append(cand)
            lists.append(torch.from_numpy(cand).to(dev))
        # the same places at the lowest trials the DM-time plane leaves room for: a shallow sweep, a row's loads consecutive
        shallow = []
        for cand in hosts_lists:
            low = cand.copy()
            low[:, 0] = RQ * DQ + low[:, 0] % 8
            shallow.append(torch.from_numpy(low).to(dev))
        count = torch.tensor([ncand, 0], dtype=torch.int32, device=dev)
        fts = [torch.zeros(ncand * NF * NX, dtype=torch.float32, device=dev) for _ in range(2)]
        dmts = [torch.zeros(ncand * ndm * NX, dtype=torch.float32, device=dev) for _ in range(2)]
        info = torch.zeros(ncand * 4, dtype=torch.int32, device=dev)
        rc, blocks, threads, lds, _, _ = rtlws.cutout.geometry(delays, None, [WIDTH], [BIN], NX, NF, RQ, DQ, ncand)
        assert rc == 0

        def run(i, ft=True, dmt=True, which=lists):
            plan.run(rows.data_ptr(), NCHAN, series.data_ptr(), NSAMP, NSAMP, which[i % NSETS].data_ptr(), count.data_ptr(), ncand,
                     fts[i % 2].data_ptr() if ft else None, dmts[i % 2].data_ptr() if dmt else None, info.data_ptr(), stream=stream)

        span = NX * BIN
        host_rows = torch.empty((span + most, NCHAN), dtype=torch.float32, pin_memory=True)
        host_series = torch.empty((ndm, span), dtype=torch.float32, pin_memory=True)

        def copy(i):
            for t, _, _, at, _, _, _, _ in hosts_lists[i % NSETS]:
                n0 = int(at) + WIDTH // 2 - (NX // 2) * BIN
                need = span + int(delays[t].max())
                host_rows[:need].copy_(rows[n0:n0 + need], non_blocking=True)
                host_series.copy_(series[int(t) - RQ * DQ:int(t) + RQ * DQ + 1:DQ, n0:n0 + span], non_blocking=True)

        times = timed({"both": run, "band-time": lambda i: run(i, dmt=False), "shallow": lambda i: run(i, dmt=False, which=shallow),
                       "DM-time": lambda i: run(i, ft=False), "copy": copy},
                      {"both": steps, "band-time": steps, "shallow": steps, "DM-time": steps, "copy": 2})
        torch.cuda.synchronize()
        inside = info.cpu().numpy().reshape(ncand, 4)
        assert np.all(inside[:, 2] == 1) and np.all(inside[:, 3] == span)
        nominal = ncand * NX * BIN * NCHAN * 4
        copied = sum(ncand * (span + int(np.mean([delays[t].max() for t in c[:, 0]]))) * NCHAN * 4 + ncand * ndm * span * 4 for c in hosts_lists) / NSETS
        tb, tf, tg, tc = times["both"], times["band-time"], times["DM-time"], times["copy"]
        say("%d candidates: workgroups %s of %s threads, LDS %s B" % (ncand, blocks, threads, lds))
        say("    rtlws_cutout_run  %9.1f .. %9.1f us/run   (%s)" % (min(tb), max(tb), " ".join("%.1f" % x for x in tb)))
        say("      band-time alone %9.1f .. %9.1f us/run   nx b nchan 4 = %.1f MB over it: %.3f .. %.3f of the HBM peak  (%s)"
            % (min(tf), max(tf), nominal / 1e6, nominal / max(tf) * 1e6 / HBM_PEAK, nominal / min(tf) * 1e6 / HBM_PEAK, " ".join("%.1f" % x for x in tf)))
        tl = times["shallow"]
        say("      at trials %d .. %d %9.1f .. %9.1f us/run   (sweeps of at most %d rows) %.3f .. %.3f of the HBM peak  (%s)"
            % (RQ * DQ, RQ * DQ + 7, min(tl), max(tl), int(delays[RQ * DQ + 7].max()), nominal / max(tl) * 1e6 / HBM_PEAK, nominal / min(tl) * 1e6 / HBM_PEAK,
               " ".join("%.1f" % x for x in tl)))
        say("      DM-time alone   %9.1f .. %9.1f us/run   (%s)" % (min(tg), max(tg), " ".join("%.1f" % x for x in tg)))
        say("    copy to the host  %9.1f .. %9.1f us       = %.1f times the run's median; %.1f MB a list, %.1f GB/s; the ranges %s  (%s)"
            % (min(tc), max(tc), float(np.median(tc)) / float(np.median(tb)), copied / 1e6, copied / float(np.median(tc)) / 1e3,
               "do not overlap" if min(tc) > max(tb) else "OVERLAP", " ".join("%.1f" % x for x in tc)))
        del lists, fts, dmts, info, host_rows, host_series

    plan.close()
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
