#!/usr/bin/env python3
"""Single-pulse search on device-resident series: one launch of rtlws_pulse_run (include/rtlws_pulse.h) per shape against
a straightforward form of the same sums and peaks in the same process (tools/variants/pulse_direct.hip: one thread per
(trial, width, n) adding its samples from device memory in the balanced order with a carry stack, no LDS, and a second
kernel for the peaks), which is this kernel's only yardstick so far.

    python tools/pulse_rates.py [--out FILE]      256 trials x 8192 and x 65 536 outputs, the ladder 1, 2, 4, .., 1024,
                                                  seg 4096; the same with a table of sixteen mixed widths; device
                                                  events, one process, three alternating rounds

The method is tools/dedisp_rates.py's: every round times `steps` launches between two events; consecutive launches read
and write different buffers (two sets of series, two sets of outputs).  Before a shape is timed the two forms' peaks and
places are compared on the device, bit for bit.  Per shape: microseconds per launch of the product with and without the
moments and of the direct form, min .. max of the rounds; for the product the boxcar outputs per second and the LDS
accesses of its levels and pieces (4 bytes each) as a fraction of 128 bytes per clock per compute unit on 256 units at
2.4 GHz.  The lines go to FILE (default profiles/pulse_rates.txt) and to stdout.  The comparison form is compiled on first
use (hipcc) into rtl-ws_amd/lib/variants/pulse_direct.so."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

LDS_PEAK = 256 * 128 * 2.4e9                    # bytes per second: ds_read_b32 / ds_write_b32 on every compute unit
LADDER = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
MIXED16 = (1, 2, 3, 5, 7, 12, 20, 33, 60, 100, 180, 255, 257, 511, 1000, 1023)
SEG = 4096


def direct_lib():
    src = os.path.join(ROOT, "tools", "variants", "pulse_direct.hip")
    out = os.path.join(ROOT, "rtl-ws_amd", "lib", "variants", "pulse_direct.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared",
                        "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.pulse_direct.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]
    return lib


def lds_accesses(widths, tile, seg, nout):
    """LDS words the product reads and writes per trial: per tile of a segment the staged samples, three accesses per
    entry of every level above 0, and one read per piece and output"""
    w_max, top = max(widths), max(widths).bit_length() - 1
    pieces = sum(bin(w).count("1") for w in widths)
    total = 0
    for s0 in range(0, nout, seg):
        length = min(seg, nout - s0)
        for j0 in range(0, length, tile):
            cnt = min(tile, length - j0)
            total += cnt + w_max - 1 + sum(3 * (cnt + w_max - (1 << l)) for l in range(1, top + 1)) + pieces * cnt
    return total


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "pulse_rates.txt")
    if args and args[0] == "--out":
        out_path = args[1]

    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    D = direct_lib()
    stream = rtlws.torch_stream_handle()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("f32 series on the device; rtlws_pulse_run against tools/variants/pulse_direct.hip (one thread per (trial, width, n), no LDS, "
        "a second kernel for the peaks) in one process; device events, three alternating rounds, two sets of series and of outputs in "
        "turn; LDS peak taken as %.1f TB/s (128 B per clock per compute unit, 256 units, 2.4 GHz)" % (LDS_PEAK / 1e12))
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

    ntrials = 256
    for tag, widths in (("ladder 1 .. 1024", LADDER), ("16 mixed widths", MIXED16)):
        for nout in (8192, 65536):
            rc, blocks, threads, lds, tile, kept, nseg = rtlws.pulse_geometry(widths, SEG, ntrials, nout)
            assert rc == 0
            plan = rtlws.PulsePlan.open(eng, widths, SEG)
            need = plan.samples_needed(nout)
            stride = (need + 3) // 4 * 4
            nw = len(widths)
            series = [torch.randn((ntrials, stride), dtype=torch.float32, device=dev) for _ in range(2)]
            peaks = [torch.empty(ntrials * nw * nseg, dtype=torch.float32, device=dev) for _ in range(3)]
            ats = [torch.empty(ntrials * nw * nseg, dtype=torch.int32, device=dev) for _ in range(3)]
            moms = [torch.empty(ntrials * nseg * 2, dtype=torch.float64, device=dev) for _ in range(2)]
            sums = torch.empty(ntrials * nw * nout, dtype=torch.float32, device=dev)
            d_widths = torch.tensor(widths, dtype=torch.int32, device=dev)

            def product(i, o=None, mom=True):
                o = i % 2 if o is None else o
                plan.run(series[i % 2].data_ptr(), stride, ntrials, nout, peaks[o].data_ptr(), ats[o].data_ptr(),
                         moms[i % 2].data_ptr() if mom else None, stream=stream)

            def direct(i, o=None):
                o = i % 2 if o is None else o
                rc = D.pulse_direct(series[i % 2].data_ptr(), stride, ntrials, nout, d_widths.data_ptr(), nw, SEG, sums.data_ptr(),
                                    peaks[o].data_ptr(), ats[o].data_ptr(), stream)
                assert rc == 0, rc

            product(0, 2)
            direct(0, 1)
            torch.cuda.synchronize()
            assert torch.equal(peaks[2].view(torch.int32), peaks[1].view(torch.int32)) and torch.equal(ats[2], ats[1]), "the two forms differ"
            heavy = nout > 8192
            times = timed({"product": product, "peaks only": lambda i: product(i, mom=False), "direct": direct},
                          {"product": 20, "peaks only": 20, "direct": 3 if heavy else 20})
            tp, tn, td = times["product"], times["peaks only"], times["direct"]
            outputs = ntrials * nw * nout
            words = ntrials * lds_accesses(widths, tile, SEG, nout)
            say("%s  %d trials x %d outputs, seg %d: tile %d, %d levels kept, %d B LDS, %d workgroups" % (tag, ntrials, nout, SEG, tile, kept, lds, blocks))
            say("    rtlws_pulse_run   %9.1f .. %9.1f us/launch  %6.2f .. %6.2f G boxcar outputs/s  = %.3f .. %.3f of the LDS peak  (%s)"
                % (min(tp), max(tp), outputs / max(tp) / 1e3, outputs / min(tp) / 1e3, 4 * words / max(tp) * 1e6 / LDS_PEAK,
                   4 * words / min(tp) * 1e6 / LDS_PEAK, " ".join("%.1f" % x for x in tp)))
            say("    ... d_mom NULL    %9.1f .. %9.1f us/launch  (%s)" % (min(tn), max(tn), " ".join("%.1f" % x for x in tn)))
            say("    direct form       %9.1f .. %9.1f us/launch  = %.1f times the product's median, %.1f times without moments; the ranges %s  (%s)"
                % (min(td), max(td), float(np.median(td)) / float(np.median(tp)), float(np.median(td)) / float(np.median(tn)),
                   "do not overlap" if min(td) > max(tp) else "OVERLAP", " ".join("%.1f" % x for x in td)))
            plan.close()
            del series, peaks, ats, moms, sums

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
