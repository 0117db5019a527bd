#!/usr/bin/env python3
"""Epoch folding on device-resident series: one launch of rtlws_fold_run (include/rtlws_fold.h) per shape against a direct
form of the same sums in the same process (tools/variants/fold_direct.hip: one thread per (trial, period,
sub-integration) with its profile in device memory, no LDS), which is this kernel's only yardstick so far, and against
the product's own kernel with the other epilogue (tools/variants/fold_transposed.hip: the histogram read transposed,
taking the bank conflicts, and stored in whole rows).

    python tools/fold_rates.py [--out FILE]      64 trials x 2^18 samples, 1024 periods, 64 and 256 bins,
                                                 sub-integrations of 2^14 and 2^18 samples; device events, one
                                                 process, three alternating rounds

The method is tools/pulse_rates.py's: every round times `steps` launches between two events; consecutive launches read
and write different buffers (two sets of series, two sets of outputs).  Before a shape is timed the three forms'
profiles (and the two kernels' hits) are compared on the device, bit for bit.  Per shape: microseconds per launch of the
product with and without the hits, of the transposed epilogue and of the direct form, min .. max of the rounds; for the
product the (sample, period) additions per second and that rate as a fraction of the LDS rate of one 4-byte
read-modify-write per lane, taken (not measured) as ds_write_b32's 64 bytes per clock per compute unit -- the add moves an
address and a data register to the LDS like a store -- on 256 units at 2.4 GHz.  The lines go to FILE (default
profiles/fold_rates.txt) and to stdout.  The comparison forms are compiled on first use (hipcc) into
rtl-ws_amd/lib/variants/."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

LDS_ADDS_PEAK = 256 * (64 / 4) * 2.4e9          # additions per second: 64 B per clock per compute unit, 4 bytes each
NTRIALS, NPERIODS, NSAMP = 64, 1024, 1 << 18


def variant_lib(name, argtypes):
    src = os.path.join(ROOT, "tools", "variants", name + ".hip")
    out = os.path.join(ROOT, "rtl-ws_amd", "lib", "variants", name + ".so")
    newest = max(os.path.getmtime(f) for f in (src, os.path.join(ROOT, "rtl-ws_amd", "csrc", "fold_kernel.h"), os.path.join(ROOT, "rtl-ws_amd", "csrc", "fold.h")))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared",
                        "-ffp-contract=fast", "-fno-slp-vectorize", "-I", os.path.join(ROOT, "rtl-ws_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        "-o", out, src], check=True)
    lib = C.CDLL(out)
    getattr(lib, name).argtypes = argtypes
    return lib


def variant_libs():
    head = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p]
    return variant_lib("fold_direct", head + [C.c_void_p]), variant_lib("fold_transposed", head + [C.c_void_p, C.c_void_p])


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "fold_rates.txt")
    if args and args[0] == "--out":
        out_path = args[1]
    if args and args[0] == "--build":                       # compile the comparison forms and stop (no GPU needed)
        variant_libs()
        return

    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    D, X = variant_libs()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("f32 series on the device; rtlws_fold_run against tools/variants/fold_direct.hip (one thread per (trial, period, sub-integration), "
        "its profile in device memory, no LDS) and tools/variants/fold_transposed.hip (the product's kernel with the transposed epilogue) in "
        "one process; device events, three alternating rounds, two sets of series and of outputs in turn; the LDS rate of one 4-byte "
        "read-modify-write per lane taken, not measured, as %.2f T additions/s (ds_write_b32's 64 B per clock per compute unit in the guide's "
        "LDS table, 256 units, 2.4 GHz)" % (LDS_ADDS_PEAK / 1e12))
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()

    def timed(fns, steps):
        times = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                fn(0), fn(1)
                H.rtlws_event_record(e0, eng.h, stream)
                for i in range(steps[name]):
                    fn(i)
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / steps[name])
        return times

    rng = np.random.default_rng(1)
    periods = 50.0 + 0.173 * np.arange(NPERIODS)             # non-dyadic, 50 .. 227 samples
    steps_h = np.array([rtlws.fold_step(p) for p in periods], np.uint64)
    phases_h = rng.integers(0, 1 << 64, NPERIODS, dtype=np.uint64)
    d_steps = torch.from_numpy(steps_h.view(np.int64)).to(dev)
    d_phases = torch.from_numpy(phases_h.view(np.int64)).to(dev)
    series = [torch.randn((NTRIALS, NSAMP), dtype=torch.float32, device=dev) for _ in range(2)]
    for nbins in (64, 256):
        for sub in (1 << 14, 1 << 18):
            rc, blocks, threads, lds, tile, wpb, nsub = rtlws.fold_geometry(NPERIODS, nbins, sub, NTRIALS, NSAMP)
            assert rc == 0
            plan = rtlws.FoldPlan.open(eng, steps_h, phases_h, nbins, sub)
            profs = [torch.empty(NTRIALS * NPERIODS * nsub * nbins, dtype=torch.float32, device=dev) for _ in range(4)]
            hits = [torch.zeros(NPERIODS * nsub * nbins, dtype=torch.int32, device=dev) for _ in range(3)]

            def product(i, o=None, want_hits=True):
                o = i % 2 if o is None else o
                plan.run(series[i % 2].data_ptr(), NSAMP, NTRIALS, NSAMP, profs[o].data_ptr(), hits[o % 3].data_ptr() if want_hits else None, stream=stream)

            def transposed(i, o=None):
                o = i % 2 if o is None else o
                rc = X.fold_transposed(series[i % 2].data_ptr(), NSAMP, NTRIALS, NSAMP, d_steps.data_ptr(), d_phases.data_ptr(), NPERIODS, nbins, sub,
                                       profs[o].data_ptr(), hits[o % 3].data_ptr(), stream)
                assert rc == 0, rc

            def direct(i, o=None):
                o = i % 2 if o is None else o
                rc = D.fold_direct(series[i % 2].data_ptr(), NSAMP, NTRIALS, NSAMP, d_steps.data_ptr(), d_phases.data_ptr(), NPERIODS, nbins, sub,
                                   profs[o].data_ptr(), stream)
                assert rc == 0, rc

            product(0, 2)
            direct(0, 3)
            torch.cuda.synchronize()
            assert torch.equal(profs[2].view(torch.int32), profs[3].view(torch.int32)), "the product and the direct form differ"
            kept = hits[2].clone()
            transposed(0, 3)
            torch.cuda.synchronize()
            assert torch.equal(profs[2].view(torch.int32), profs[3].view(torch.int32)), "the two epilogues' profiles differ"
            assert torch.equal(kept, hits[0]) and int(kept.sum()) == NPERIODS * NSAMP, "the two epilogues' hits differ"
            times = timed({"product": product, "no hits": lambda i: product(i, want_hits=False), "transposed": transposed, "direct": direct},
                          {"product": 10, "no hits": 10, "transposed": 10, "direct": 2})
            tp, tn, tx, td = times["product"], times["no hits"], times["transposed"], times["direct"]
            adds = NTRIALS * NPERIODS * NSAMP
            say("%d bins, sub %d  %d trials x %d samples, %d periods: %d waves per workgroup, %d B LDS, %d workgroups, %d sub-integrations"
                % (nbins, sub, NTRIALS, NSAMP, NPERIODS, wpb, lds, blocks, nsub))
            say("    rtlws_fold_run    %10.1f .. %10.1f us/launch  %6.3f .. %6.3f T additions/s  = %.3f .. %.3f of the LDS rate  (%s)"
                % (min(tp), max(tp), adds / max(tp) / 1e6, adds / min(tp) / 1e6, adds / max(tp) * 1e6 / LDS_ADDS_PEAK,
                   adds / min(tp) * 1e6 / LDS_ADDS_PEAK, " ".join("%.1f" % x for x in tp)))
            say("    ... d_hits NULL   %10.1f .. %10.1f us/launch  (%s)" % (min(tn), max(tn), " ".join("%.1f" % x for x in tn)))
            say("    transposed epilogue %8.1f .. %10.1f us/launch  = %.4f times the product's median; the ranges %s  (%s)"
                % (min(tx), max(tx), float(np.median(tx)) / float(np.median(tp)),
                   "do not overlap" if min(tx) > max(tp) or max(tx) < min(tp) else "overlap", " ".join("%.1f" % x for x in tx)))
            say("    direct form       %10.1f .. %10.1f us/launch  = %.1f times the product's median, %.1f times without hits; the ranges %s  (%s)"
                % (min(td), max(td), float(np.median(td)) / float(np.median(tp)), float(np.median(td)) / float(np.median(tn)),
                   "do not overlap" if min(td) > max(tp) else "OVERLAP", " ".join("%.1f" % x for x in td)))
            plan.close()
            del profs, hits

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
