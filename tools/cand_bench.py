#!/usr/bin/env python3
"""Candidate folding on a device-resident waterfall (include/rtlws_cand.h): the time of rtlws_cand_fold_run at 1024
channels x 2^17 rows, 8 candidates behind dispersion sweeps, 128 bins, sub-integrations of 4096 rows; of the two stages of
rtlws_cand_search_run at 65 DM trials x 129 period trials over that cube; and of the only other route to the same cube,
rtlws_fold_run over a channel-major copy of the waterfall with one trial per channel and one period.

    python tools/cand_bench.py [--out FILE]    device events around the launches only, one process, three alternating
                                               rounds; the lines go to FILE (default profiles/cand.txt) and to stdout

The cube's algorithmic bytes: every candidate reads the nsamp rows once (4 nchan bytes each) and the cube is written once.
The HBM peak is taken, not measured, as 8.0 TB/s (the guide's chip table).  rtlws_cand_search_run is two launches behind
one call: stage 1 is timed through a plan of one period trial (its stage 2 is then ncand * ndm workgroups of one live
wavefront and 32 sub-integrations), and stage 2 as the whole run less that."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12
NCHAN, NSAMP, NCAND, NBINS, SUB, NDM, NTR = 1024, 1 << 17, 8, 128, 4096, 65, 129
BAND = (NCHAN, 1, 400e6, 100e6, 1e-3)            # rtlws_dedisp_delays' description: 350 .. 450 MHz, rows of 1 ms
PERIOD = 89.7                                    # rows


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "cand.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]

    import torch
    import rtlws
    import rtlws.cand as cand
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

    def span(t):
        return "%9.1f .. %9.1f us/run" % (min(t), max(t)), "(%s)" % " ".join("%.1f" % x for x in t)

    say("f32 rows on the device; device events around the launches only, three alternating rounds, two sets of inputs and of outputs in "
        "turn; the HBM peak taken, not measured, as %.1f TB/s" % (HBM_PEAK / 1e12))
    delays = rtlws.dedisp_delays(*BAND, NCAND, 20.0, 10.0)
    most = int(delays.max())
    nsub = NSAMP // SUB
    say("workload: %d channels x %d rows, %d candidates at DM 20 .. 90 (delays up to %d rows), periods from %.1f rows, %d bins, "
        "sub-integrations of %d rows (%d of them)" % (NCHAN, NSAMP, NCAND, most, PERIOD, NBINS, SUB, nsub))
    rows = [torch.randn((NSAMP + most, NCHAN), dtype=torch.float32, device=dev) for _ in range(2)]
    cubes = [torch.empty((NCAND, nsub, NCHAN, NBINS), dtype=torch.float32, device=dev) for _ in range(2)]
    hits = torch.empty((NCAND, nsub, NBINS), dtype=torch.int32, device=dev)
    steps = np.array([rtlws.fold_step(PERIOD + 3.1 * c) for c in range(NCAND)], np.uint64)
    phases = np.zeros(NCAND, np.uint64)

    # ---- the cube ----
    plan = cand.CandFoldPlan(eng, steps, phases, NCHAN, NBINS, SUB, delays)
    one = cand.CandFoldPlan(eng, steps[:1], phases[:1], NCHAN, NBINS, SUB)
    rc, blocks, threads, lds, wpb, _ = cand.fold_geometry(NCAND, NCHAN, NBINS, SUB, NSAMP)
    assert rc == 0
    fns = {
        "cube, 8 candidates": lambda i: plan.run(rows[i % 2].data_ptr(), NCHAN, NSAMP, cubes[i % 2].data_ptr(), stream=stream),
        "cube and hits": lambda i: plan.run(rows[i % 2].data_ptr(), NCHAN, NSAMP, cubes[i % 2].data_ptr(), hits.data_ptr(), stream=stream),
        "cube, 1 candidate, no delays": lambda i: one.run(rows[i % 2].data_ptr(), NCHAN, NSAMP, cubes[i % 2].data_ptr(), stream=stream),
    }
    times = timed(fns, 5)
    say("rtlws_cand_fold_run: %d workgroups of %d threads (%d wavefronts), LDS %d B" % (blocks, threads, wpb, lds))
    for name, ncand in (("cube, 8 candidates", NCAND), ("cube and hits", NCAND), ("cube, 1 candidate, no delays", 1)):
        t = times[name]
        nbytes = float(ncand) * (4.0 * NCHAN * NSAMP + 4.0 * nsub * NCHAN * NBINS)
        say("    %-30s %s  %7.1f MB of algorithmic bytes = %.3f .. %.3f of the HBM peak  %s"
            % ((name, span(t)[0], nbytes / 1e6, nbytes / (max(t) * 1e-6) / HBM_PEAK, nbytes / (min(t) * 1e-6) / HBM_PEAK, span(t)[1])))
    t_one = times["cube, 1 candidate, no delays"]

    # ---- the parent's route to the cube of one candidate: the channels as the trials of rtlws_fold_run ----
    series = [r[:NSAMP].t().contiguous() for r in rows]                          # channel-major copies [nchan, nsamp]
    fplan = rtlws.FoldPlan(eng, steps[:1], phases[:1], NBINS, SUB)
    prof = torch.empty((NCHAN, 1, nsub, NBINS), dtype=torch.float32, device=dev)
    t_fold = timed({"fold": lambda i: fplan.run(series[i % 2].data_ptr(), NSAMP, NCHAN, NSAMP, prof.data_ptr(), None, stream=stream)}, 3)["fold"]
    one.run(rows[0].data_ptr(), NCHAN, NSAMP, cubes[0].data_ptr(), stream=stream)
    fplan.run(series[0].data_ptr(), NSAMP, NCHAN, NSAMP, prof.data_ptr(), None, stream=stream)
    torch.cuda.synchronize()
    same = torch.equal(cubes[0][0].permute(1, 0, 2).contiguous().view(torch.int32), prof[:, 0].contiguous().view(torch.int32))
    say("the same cube of one candidate at zero delays through rtlws_fold_run (a channel-major copy of the waterfall, %d trials, one period; "
        "the copy is not timed): %s %s; the same bits: %s" % ((NCHAN,) + span(t_fold) + (same,)))
    say("    ratio rtlws_fold_run / rtlws_cand_fold_run: %.1f .. %.1f" % (min(t_fold) / max(t_one), max(t_fold) / min(t_one)))
    fplan.close()
    one.close()
    del series, prof

    # ---- the refinement over that cube ----
    plan.run(rows[0].data_ptr(), NCHAN, NSAMP, cubes[0].data_ptr(), stream=stream)
    plan.run(rows[1].data_ptr(), NCHAN, NSAMP, cubes[1].data_ptr(), stream=stream)
    a = np.stack([cand.dm_shifts(*BAND, PERIOD + 3.1 * c, NBINS, NDM, -8.0, 0.25) for c in range(NCAND)])
    g = np.stack([cand.drift_shifts(NBINS, SUB, nsub, NTR, -64 * 0.5 / NSAMP, 0.5 / NSAMP) for _ in range(NCAND)])
    both = cand.CandSearchPlan(eng, NCAND, nsub, NCHAN, NBINS, a, g)
    first = cand.CandSearchPlan(eng, NCAND, nsub, NCHAN, NBINS, a, g[:, :1])
    rc, b1, b2, threads, lds1, lds2, work = cand.search_geometry(NCAND, nsub, NCHAN, NBINS, NDM, NTR)
    assert rc == 0
    stat = [torch.empty((NCAND, NDM, NTR), dtype=torch.float64, device=dev) for _ in range(2)]
    total = [torch.empty((NCAND, NDM, NTR), dtype=torch.float64, device=dev) for _ in range(2)]
    profs = torch.empty((NCAND, NDM, NTR, NBINS), dtype=torch.float32, device=dev)
    fns = {
        "both stages": lambda i: both.run(cubes[i % 2].data_ptr(), stat[i % 2].data_ptr(), total[i % 2].data_ptr(), stream=stream),
        "both stages, P written": lambda i: both.run(cubes[i % 2].data_ptr(), stat[i % 2].data_ptr(), total[i % 2].data_ptr(), profs.data_ptr(), stream=stream),
        "stage 1 (one period trial)": lambda i: first.run(cubes[i % 2].data_ptr(), stat[i % 2].data_ptr(), total[i % 2].data_ptr(), stream=stream),
    }
    times = timed(fns, 5)
    say("rtlws_cand_search_run, %d DM trials x %d period trials: stage 1 %d workgroups of %d threads, LDS %d B; stage 2 %d workgroups, LDS %d B; "
        "workspace %.1f MB" % (NDM, NTR, b1, threads, lds1, b2, lds2, work / 1e6))
    for name in fns:
        say("    %-30s %s  %s" % ((name,) + span(times[name])))
    t_both, t_first = times["both stages"], times["stage 1 (one period trial)"]
    cube_bytes = 4.0 * NCAND * nsub * NCHAN * NBINS
    say("    stage 1 reads the cube (%.1f MB) once per group of 8 DM trials, %d times: %.1f MB = %.3f .. %.3f of the HBM peak were they all to "
        "come from memory" % (cube_bytes / 1e6, -(-NDM // 8), cube_bytes * -(-NDM // 8) / 1e6, cube_bytes * -(-NDM // 8) / (max(t_first) * 1e-6) / HBM_PEAK,
                              cube_bytes * -(-NDM // 8) / (min(t_first) * 1e-6) / HBM_PEAK))
    say("    stage 2 as the difference: %.1f .. %.1f us" % (min(t_both) - max(t_first), max(t_both) - min(t_first)))
    for p in (plan, both, first):
        p.close()
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
