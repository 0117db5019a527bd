#!/usr/bin/env python3
"""Up to 32 FM stations from one device-resident capture: one launch of rtlws_fmbank_run (include/rtlws_fmbank.h)
against the composition it is defined by, one rtlws_ddc_run plus C x rtlws_fm_audio_blocks through a
[C, dec_len] cmplx_s32 buffer in device memory.

    python tools/fmbank_rates.py --baseline LIBDIR [--samples LOG2] [--out FILE]
        LIBDIR holds the PARENT commit's libraries (librtlws_hip.so, librtlws_ddc.so, librtlws_fm.so built into a
        scratch directory): the composition runs from those, the fused side from this tree's rtl-ws_amd/lib.  The
        code under test is never the baseline.
    python tools/fmbank_rates.py --child fused|composition LIBDIR JSON STEPS LOG2      (what the driver starts)

Each side runs in a process of its own, the two alternating: first one pass of each that only computes (a position-
weighted checksum of the audio and the states of every cell, compared before anything is timed), then three rounds of
fused, composition.  A round times STEPS = 20 launches per cell between two device events after two untimed ones;
consecutive launches use different buffer sets (three captures, two sets of everything written), so no launch finds
its input or output lines in a cache.  Cells: R = 8, 10, 12 x C = 1, 8, 32 over the largest whole number of blocks
of 16 384 decimated samples in 2^LOG2 cmplx_u8 samples, and one short call (one block of 19 200 decimated samples,
C = 32) per R.  The table goes to FILE (default profiles/fmbank_rates.txt) and to stdout."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

FACTORS, CHANNELS, BLOCK_LEN, SHORT_LEN = (8, 10, 12), (1, 8, 32), 16384, 19200


def cells(log2):
    out = [(R, C, BLOCK_LEN, ((1 << log2) // R) // BLOCK_LEN) for R in FACTORS for C in CHANNELS]
    return out + [(R, 32, SHORT_LEN, 1) for R in FACTORS]


def child(side, libdir, json_path, steps, log2):
    import torch
    import rtlws
    for attr, name in (("HIP_LIB", "librtlws_hip.so"), ("DDC_LIB", "librtlws_ddc.so"), ("FM_LIB", "librtlws_fm.so"),
                       ("FMBANK_LIB", "librtlws_fmbank.so")):
        setattr(rtlws, attr, os.path.join(libdir, name))
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    if side == "fused":
        plan = rtlws.FmBankPlan.open(eng)
    else:
        plan = rtlws.DdcPlan.open(eng)
        F = rtlws.fm_lib()
        assert F.rtlws_fm_prepare(eng.h) == 0, rtlws.fm_last_error()
    torch.manual_seed(1)
    srcs = [torch.randint(0, 256, (1 << log2, 2), dtype=torch.uint8, device=dev) for _ in range(3)]
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()
    rng = np.random.default_rng(1)
    result = {}
    for R, C, L, nb in cells(log2):
        words = [12345] + [int(k) for k in rng.integers(-32768, 32768, C - 1)]
        dec_len, n = nb * L, nb * (L // 4)
        st_in = torch.rand((C, 21), dtype=torch.float32, device=dev) * 2 - 1
        st_out = [torch.zeros((C, 21), dtype=torch.float32, device=dev) for _ in range(2)]
        audio = [torch.zeros((C, n), dtype=torch.float32, device=dev) for _ in range(2)]
        if side == "composition":
            inter = [torch.empty((C, dec_len, 2), dtype=torch.int32, device=dev) for _ in range(2)]

        def launch(i):
            src, a, s = srcs[i % 3].data_ptr(), audio[i % 2].data_ptr(), st_out[i % 2].data_ptr()
            if side == "fused":
                plan.run(R, src, L, nb, words, st_in.data_ptr(), s, a, audio_stride=n, stream=stream)
            else:
                d = inter[i % 2].data_ptr()
                plan.run(R, src, dec_len, words, d, stream=stream)
                for c in range(C):
                    rc = F.rtlws_fm_audio_blocks(eng.h, d + c * dec_len * 8, L, nb, st_in.data_ptr() + c * 84, s + c * 84, 1,
                                                 a + c * n * 4, stream)
                    assert rc == 0, rtlws.fm_last_error()

        launch(0)
        torch.cuda.synchronize()
        w = (torch.arange(n, device=dev, dtype=torch.int64) % 65521) + 1
        digest = [int((audio[0].view(torch.int32).to(torch.int64) * w).sum().item()),
                  int(audio[0].view(torch.int32).to(torch.int64).sum().item()),
                  int((st_out[0].view(torch.int32).to(torch.int64) * w[:21]).sum().item())]
        del w
        us = None
        if steps:
            launch(1), launch(2)
            H.rtlws_event_record(e0, eng.h, stream)
            for i in range(steps):
                launch(i)
            H.rtlws_event_record(e1, eng.h, stream)
            torch.cuda.synchronize()
            us = 1e3 * H.rtlws_event_elapsed_ms(e0, e1) / steps
        result["%d,%d,%d,%d" % (R, C, L, nb)] = {"us": us, "digest": digest}
        del st_out, audio
        if side == "composition":
            del inter
        torch.cuda.empty_cache()
    H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    plan.close()
    eng.close()
    with open(json_path, "w") as f:
        json.dump(result, f)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], args[2], args[3], int(args[4]), int(args[5]))
    log2, out_path, baseline, steps = 27, os.path.join(ROOT, "profiles", "fmbank_rates.txt"), None, 20
    while args:
        if args[0] == "--samples":
            log2 = int(args[1])
        elif args[0] == "--out":
            out_path = args[1]
        elif args[0] == "--baseline":
            baseline = args[1]
        else:
            raise SystemExit(__doc__)
        args = args[2:]
    if not baseline:
        raise SystemExit(__doc__)
    libdirs = {"fused": os.path.join(ROOT, "rtl-ws_amd", "lib"), "composition": os.path.abspath(baseline)}
    assert not os.path.exists(os.path.join(libdirs["composition"], "librtlws_fmbank.so")), "the baseline is the parent's build"

    def run(side, nsteps):
        with tempfile.NamedTemporaryFile(suffix=".json") as tf:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, libdirs[side], tf.name, str(nsteps),
                            str(log2)], check=True, timeout=600)
            return json.load(open(tf.name))

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("%d cmplx_u8 samples on the device, blocks of %d decimated samples; fused = one rtlws_fmbank_run, composition = one "
        "rtlws_ddc_run + C x rtlws_fm_audio_blocks from the parent commit's libraries; a process per side and round, "
        "alternating, %d launches per round on rotating buffer sets, device events" % (1 << log2, BLOCK_LEN, steps))
    first = {side: run(side, 0) for side in ("fused", "composition")}
    for key in first["fused"]:
        assert first["fused"][key]["digest"] == first["composition"][key]["digest"], "audio or states differ at " + key
    say("audio and states of the two sides: equal checksums in all %d cells, compared before timing" % len(first["fused"]))
    times = {"fused": {}, "composition": {}}
    for _ in range(3):
        for side in ("fused", "composition"):
            for key, v in run(side, steps).items():
                assert v["digest"] == first[side][key]["digest"], key
                times[side].setdefault(key, []).append(v["us"])
    for R, C, L, nb in cells(log2):
        key = "%d,%d,%d,%d" % (R, C, L, nb)
        f, c = times["fused"][key], times["composition"][key]
        dec = nb * L
        verdict = "confirmed" if max(f) < min(c) else "refuted"
        say("R=%-2d C=%-2d %5d x %5d  fused %8.1f .. %8.1f us (%s)  composition %8.1f .. %8.1f us (%s)  composition / fused "
            "= %.2f (medians), bytes bound (2R + 17C) / (2R + C) = %.2f; fused %.0f GB/s at 2R + C bytes; fused range "
            "wholly below: %s" % (R, C, nb, L, min(f), max(f), " ".join("%.1f" % x for x in f), min(c), max(c),
                                  " ".join("%.1f" % x for x in c), float(np.median(c) / np.median(f)),
                                  (2 * R + 17 * C) / (2 * R + C), dec * (2 * R + C) / float(np.median(f)) / 1e3, verdict))
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
