#!/usr/bin/env python3
"""Incoherent dedispersion on device-resident rows: one launch of rtlws_dedisp_run (include/rtlws_dedisp.h) per shape
against a straightforward form of the same sum in the same process (tools/variants/dedisp_direct.hip: one thread per
output, every term read from device memory, no LDS), which is this kernel's only yardstick so far.

    python tools/dedisp_rates.py [--out FILE]      M = 1024 and 64, 256 trials of rtlws_dedisp_delays (408 MHz centre,
                                                   2.4 MHz, 0.8533 ms rows, DM 0, 0.5, ..), 8192 and 65 536 rows; one
                                                   table of random delays up to 5000 rows (M = 64, 32 trials, 8192 rows);
                                                   device events, one process, three alternating rounds

The method is tools/pfbspec_rates.py's: every round times `steps` launches between two events; consecutive launches read
and write different buffers (two sets of rows, two outputs).  Before a shape is timed the two forms' outputs are compared
on the device, bit for bit.  Per shape: microseconds per launch of both forms, min .. max of the rounds; for the product
form the additions per second, the bytes its loads ask for (from the plan: every trial group of every tile stages, per
four neighbouring positions, 256 rows and the spread of their delays, 16 bytes each; the lone form a whole quad per
position) over the algorithmic 4 rows M + 4 ntrials nout, and the additions' LDS reads (4 bytes each, ds_read_b32) as a
fraction of 128 bytes per clock per compute unit on 256 units at 2.4 GHz.  The lines go to FILE (default
profiles/dedisp_rates.txt) and to stdout.  The comparison form is compiled on first use (hipcc) into
rtl-ws_amd/lib/variants/dedisp_direct.so."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

LDS_READ_PEAK = 256 * 128 * 2.4e9               # bytes per second: ds_read_b32 on every compute unit
SWEEP = (408e6, 2.4e6, 0.8533e-3)               # centre, bandwidth, seconds per row
TILE = 256


def direct_lib():
    src = os.path.join(ROOT, "tools", "variants", "dedisp_direct.hip")
    out = os.path.join(ROOT, "rtl-ws_amd", "lib", "variants", "dedisp_direct.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared",
                        "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.dedisp_direct.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
    return lib


def requested_bytes(delays, per, nout, lone):
    """What the plan's loads ask of the memory system for nout outputs"""
    ntrials, m = delays.shape
    delays = delays.astype(np.int64)
    tiles = -(-int(nout) // TILE)
    total = 0
    for t0 in range(0, ntrials, per):
        g = delays[t0:t0 + per]
        if lone:
            total += tiles * m * TILE * 16
        else:
            q = g.reshape(g.shape[0], m // 4, 4)
            total += tiles * int((TILE + q.max(axis=(0, 2)) - q.min(axis=(0, 2))).sum()) * 16
    return total


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "dedisp_rates.txt")
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

    say("f32 rows on the device; rtlws_dedisp_run against tools/variants/dedisp_direct.hip (one thread per output, no LDS) in one "
        "process; device events, three alternating rounds, two sets of rows and two outputs in turn; LDS read peak taken as "
        "%.1f TB/s (ds_read_b32: 128 B per clock per compute unit, 256 units, 2.4 GHz)" % (LDS_READ_PEAK / 1e12))
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

    rng = np.random.default_rng(5)
    shapes = [("M=%-4d 256 trials DM 0..127.5 %6d rows" % (m, nrows), rtlws.dedisp_delays(m, 1, *SWEEP, 256, 0.0, 0.5), nrows)
              for m in (1024, 64) for nrows in (8192, 65536)]
    shapes.append(("M=64   32 trials random <= 5000  8192 rows", rng.integers(0, 5001, (32, 64)).astype(np.int32), 8192))
    for tag, delays, nrows in shapes:
        ntrials, m = delays.shape
        rc, blocks, threads, lds, tile, per, most = rtlws.dedisp_geometry(delays, None, 1)
        nout = nrows - most
        blocks = rtlws.dedisp_geometry(delays, None, nout)[1]
        lone = per == 1 and int((delays.reshape(ntrials, m // 4, 4).max(axis=2) - delays.reshape(ntrials, m // 4, 4).min(axis=2)).max()) > 3776
        plan = rtlws.DedispPlan.open(eng, delays)
        assert plan.rows_needed(nout) == nrows and tile == TILE
        rows = [torch.rand((nrows, m), dtype=torch.float32, device=dev) for _ in range(2)]
        outs = [torch.empty((ntrials, nout), dtype=torch.float32, device=dev) for _ in range(3)]
        d_delays = torch.from_numpy(delays).to(dev)

        def product(i, out=None):
            plan.run(rows[i % 2].data_ptr(), nout, (outs[i % 2] if out is None else out).data_ptr(), stream=stream)

        def direct(i, out=None):
            rc = D.dedisp_direct(rows[i % 2].data_ptr(), m, d_delays.data_ptr(), None, m, ntrials, nout,
                                 (outs[i % 2] if out is None else out).data_ptr(), nout, stream)
            assert rc == 0, rc

        product(0, outs[2])
        direct(0, outs[1])
        torch.cuda.synchronize()
        assert torch.equal(outs[2], outs[1]), "the two forms differ"
        adds = ntrials * nout * m
        heavy = adds > 1 << 32
        times = timed({"product": product, "direct": direct}, {"product": 20, "direct": 3 if heavy else 20})
        tp, td = times["product"], times["direct"]
        algorithmic = 4 * nrows * m + 4 * ntrials * nout
        asked = requested_bytes(delays, per, nout, lone) + 4 * ntrials * nout
        say("%s  %d outputs a trial, %d trials a workgroup, %d B LDS, %d workgroups" % (tag, nout, per, lds, blocks))
        say("    rtlws_dedisp_run  %9.1f .. %9.1f us/launch  %6.2f .. %6.2f T additions/s  = %.3f .. %.3f of the LDS read peak; its loads "
            "ask for %.1f times the algorithmic %.1f MB  (%s)"
            % (min(tp), max(tp), adds / max(tp) / 1e6, adds / min(tp) / 1e6, 4 * adds / max(tp) * 1e6 / LDS_READ_PEAK,
               4 * adds / min(tp) * 1e6 / LDS_READ_PEAK, asked / algorithmic, algorithmic / 1e6, " ".join("%.1f" % x for x in tp)))
        say("    direct form       %9.1f .. %9.1f us/launch  = %.1f times the product's median  (%s)"
            % (min(td), max(td), float(np.median(td)) / float(np.median(tp)), " ".join("%.1f" % x for x in td)))
        plan.close()
        del rows, outs

    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
