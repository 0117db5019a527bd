#!/usr/bin/env python3
"""Rates of the long-frame path (include/rtlws_long.h) for cmplx_u8 frames of 2^14, 2^16, 2^18 and 2^20 points,
K = 1, f64 and f32 rows, about 2^26 points per launch -- beside the yardstick, rtlws_spectra_batch_f64 at its
largest size N = 8192 on the same number of points, measured in the same process, alternating three times.

    python tools/long_frames_rates.py                 event timings, the table (stdout)
    python tools/long_frames_rates.py --cpu           ... with the oracle's 16-thread CPU rate beside it
    rocprofv3 --kernel-trace --stats -d DIR/trace --output-format csv -- python tools/long_frames_rates.py --profile-run
    rocprofv3 --pmc FETCH_SIZE -d DIR/pmc_fetch --output-format csv -- python tools/long_frames_rates.py --profile-run
    rocprofv3 --pmc WRITE_SIZE -d DIR/pmc_write --output-format csv -- python tools/long_frames_rates.py --profile-run
    python tools/long_frames_rates.py --summarize DIR   per-pass times and HBM traffic from those three runs

Contract bytes per frame: 2 N in, 8 N / K (f64 rows) or 4 N / K (f32 rows) out.  The workspace adds 16 N written
and 16 N read per frame, which the measured traffic has to show.  HBM peak: 8 TB/s."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

POINTS = 1 << 26
SIZES = (14, 16, 18, 20)
YARD_N = 8192
HBM_PEAK = 8e12


def contract_bytes(points, rows_f32):
    return points * (2 + (4 if rows_f32 else 8))


def configs(eng, rtlws, torch, dev):
    """[(label, points per launch, rows_f32, launch(i))]: the yardstick first, then the long sizes."""
    stream = rtlws.torch_stream_handle()
    src = [torch.randint(0, 256, (POINTS, 2), dtype=torch.uint8, device=dev) for _ in range(2)]
    out = torch.empty(POINTS, dtype=torch.float64, device=dev)
    cfg = []
    for rows_f32 in (False, True):
        flags = rtlws.FLAG_ROWS_F32 if rows_f32 else 0
        desc = rtlws.make_desc(YARD_N, flags=flags)
        assert rtlws.hip_lib().rtlws_engine_prepare_f64(eng.h, YARD_N) == 0
        cfg.append(("batch_f64 N=8192 %s rows" % ("f32" if rows_f32 else "f64"), POINTS, rows_f32,
                    lambda i, d=desc: eng.spectra_batch_f64(d, src[i % 2].data_ptr(), POINTS // YARD_N, out.data_ptr(),
                                                            stream=stream)))
    plans = []
    for m in SIZES:
        for rows_f32 in (False, True):
            flags = rtlws.FLAG_ROWS_F32 if rows_f32 else 0
            plan = rtlws.LongPlan(eng, rtlws.make_desc(1 << m, flags=flags), POINTS >> m)
            assert plan.workspace_bytes == 16 * POINTS          # one group
            plans.append(plan)
            cfg.append(("long N=2^%d %s rows" % (m, "f32" if rows_f32 else "f64"), POINTS, rows_f32,
                        lambda i, p=plan, f=POINTS >> m: p.run(src[i % 2].data_ptr(), f, out.data_ptr(), stream=stream)))
    return cfg, plans


def time_launches(L, eng, stream, launch, steps):
    e0, e1 = L.rtlws_event_create(), L.rtlws_event_create()
    L.rtlws_event_record(e0, eng.h, stream)
    for i in range(steps):
        launch(i)
    L.rtlws_event_record(e1, eng.h, stream)
    ms = L.rtlws_event_elapsed_ms(e0, e1) / steps
    L.rtlws_event_destroy(e0)
    L.rtlws_event_destroy(e1)
    return ms * 1e-3


def rates(with_cpu):
    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    L = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    cfg, plans = configs(eng, rtlws, torch, dev)
    for _, _, _, launch in cfg:                                  # warm up every shape
        launch(0)
        launch(1)
    torch.cuda.synchronize()
    rounds = 3
    secs = {label: [] for label, _, _, _ in cfg}
    for _ in range(rounds):                                      # alternating: every configuration once per round
        for label, _, _, launch in cfg:
            secs[label].append(time_launches(L, eng, stream, launch, 6))
    print("# %d points per launch, cmplx_u8, K = 1; device events over 6 launches, %d alternating rounds (median; min-max)"
          % (POINTS, rounds))
    print("# %-28s %10s %12s %12s %9s %s" % ("configuration", "ms/launch", "points/s", "spectra/s", "of 8 TB/s", "spread ms"))
    med = {}
    for label, points, rows_f32, _ in cfg:
        s = sorted(secs[label])
        t = s[len(s) // 2]
        med[label] = t
        n = YARD_N if "8192" in label else 1 << int(label.split("^")[1].split()[0])
        print("  %-28s %10.3f %12.4g %12.4g %9.4f %.3f-%.3f" % (label, 1e3 * t, points / t, points / n / t,
                                                               contract_bytes(points, rows_f32) / t / HBM_PEAK,
                                                               1e3 * s[0], 1e3 * s[-1]))
    print("# per point against the yardstick (rtlws_spectra_batch_f64, N = 8192, same rows): > 1 is faster")
    for label, _, rows_f32, _ in cfg:
        if label.startswith("long"):
            yard = med["batch_f64 N=8192 %s rows" % ("f32" if rows_f32 else "f64")]
            r = yard / med[label]
            print("  %-28s %.2fx%s" % (label, r, "" if r >= 1.0 else "   SLOWER per point than the yardstick"))
    if with_cpu:
        from rtlws import synth
        from oracle import pyoracle as po
        print("# the oracle on 16 CPU threads (f64, same arithmetic contract), 2^24 points per call")
        for m in SIZES:
            N = 1 << m
            frames = max((1 << 24) >> m, 16)
            iq = synth.uniform_iq(frames, N, seed=m)
            outb = np.empty((frames, N))
            po.batch_spectra_u8(iq, N, nthreads=16, out=outb)
            t0 = time.perf_counter()
            po.batch_spectra_u8(iq, N, nthreads=16, out=outb)
            t = time.perf_counter() - t0
            print("  oracle N=2^%d: %.4g points/s, %.4g spectra/s" % (m, frames * N / t, frames / t))
    for p in plans:
        p.close()
    eng.close()


def profile_run():
    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    cfg, plans = configs(eng, rtlws, torch, dev)
    for _, _, _, launch in cfg:
        for i in range(4):
            launch(i)
        torch.cuda.synchronize()
    for p in plans:
        p.close()
    eng.close()


def _rows(pattern):
    for f in glob.glob(pattern, recursive=True):
        yield from csv.DictReader(open(f))


def summarize(d):
    dur = {}
    for r in _rows(os.path.join(d, "trace", "**", "*_kernel_trace.csv")):
        if "long_pass" in r["Kernel_Name"] or "spectra_f64<" in r["Kernel_Name"]:
            dur.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    pmc = {}
    for which in ("fetch", "write"):
        for r in _rows(os.path.join(d, "pmc_" + which, "**", "*_counter_collection.csv")):
            if "long_pass" in r["Kernel_Name"] or "spectra_f64<" in r["Kernel_Name"]:
                pmc.setdefault((r["Kernel_Name"], r["Counter_Name"]), []).append(float(r["Counter_Value"]))
    short = lambda n: n.replace("void rtlws::lng::", "").replace("void rtlws::", "").split("(")[0]
    print("# rocprofv3 --kernel-trace: per kernel, launches after the first dropped; --pmc FETCH_SIZE / WRITE_SIZE in "
          "runs of their own (KiB per launch; FETCH_SIZE doubled: gfx950 counts a wide read at half its bytes,"
          " which is calibrated for 16-byte-per-lane loads only -- pass A's 2-byte loads are not)")
    print("# %-26s %8s %11s %14s %14s %s" % ("kernel", "launches", "avg ms", "read MiB", "written MiB", "of 8 TB/s"))
    for name in sorted(dur, key=short):
        v = dur[name][1:] or dur[name]
        avg = sum(v) / len(v)
        fe = pmc.get((name, "FETCH_SIZE"), [0.0])
        wr = pmc.get((name, "WRITE_SIZE"), [0.0])
        rd_b, wr_b = 2 * 1024 * sum(fe) / len(fe), 1024 * sum(wr) / len(wr)
        print("  %-26s %8d %11.4f %14.1f %14.1f %.4f" % (short(name), len(v), avg * 1e-6, rd_b / 2**20, wr_b / 2**20,
                                                      (rd_b + wr_b) / (avg * 1e-9) / HBM_PEAK))
    print("# contract bytes per launch of %d points: %.0f MiB (f64 rows), %.0f MiB (f32 rows); workspace: %.0f MiB "
          "written by pass A + %.0f MiB read by pass B" % (POINTS, contract_bytes(POINTS, False) / 2**20,
                                                          contract_bytes(POINTS, True) / 2**20, 16 * POINTS / 2**20,
                                                          16 * POINTS / 2**20))


if __name__ == "__main__":
    if "--summarize" in sys.argv:
        summarize(sys.argv[sys.argv.index("--summarize") + 1])
    elif "--profile-run" in sys.argv:
        profile_run()
    else:
        rates("--cpu" in sys.argv)
