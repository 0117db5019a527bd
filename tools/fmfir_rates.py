#!/usr/bin/env python3
"""Up to 32 FM stations from one device-resident capture behind an int16 FIR: one launch of rtlws_fmfir_run
(include/rtlws_fmfir.h) against the composition it is defined by, one rtlws_ddcfir_run plus C x rtlws_fm_audio_blocks
through a [C, dec_len] cmplx_s32 buffer in device memory, both from this tree's libraries (librtlws_fm.so's sources
are the parent commit's; librtlws_ddcfir.so's kernels and the host side of its two object files are the parent's,
instruction for instruction: profiles/fmfir_codeobj.txt); and
rtlws_fmbank_run at the same R, the price of the filter.

    python tools/fmfir_rates.py [--samples LOG2] [--out FILE]
    python tools/fmfir_rates.py --child fused|composition|unfiltered JSON STEPS LOG2      (what the driver starts)

Expectation, stated before the run: fusing removes 16 C bytes per decimated sample and C launches,
not the chain's vector work (4.13), so composition / fused may land on either side of 1 at C = 32 and lands well above 1
on the one-block short call; per cell "confirmed" means the fused range lies wholly below the composition's.

Each side runs in a process of its own, the sides alternating: first one pass of each that only computes (a position-
weighted checksum of the audio and the states of every cell; fused and composition are compared before anything is
timed), then three rounds.  A round times STEPS = 20 launches per cell between two device events after two untimed
ones; consecutive launches use different buffer sets (three captures, two sets of everything written).  Cells:
R = 8, 10, 12 with L = 8 R designed taps x C = 1, 8, 32 over the largest whole number of blocks of 16 384 decimated
samples in 2^LOG2 cmplx_u8 samples, and one short call (one block of 19 200 decimated samples, C = 32) per R.  Not
measured: hardware counters, odd R or L (the 2-byte load form; R = 10 takes the 4-byte one).  The table goes to FILE (default
profiles/fmfir_rates.txt) and to stdout."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

FACTORS, CHANNELS, BLOCK_LEN, SHORT_LEN, SHIFT = (8, 10, 12), (1, 8, 32), 16384, 19200, 14
SIDES = ("fused", "composition", "unfiltered")


def cells(log2):
    def blocks(R):
        return ((1 << log2) - 8 * R) // R // BLOCK_LEN
    out = [(R, C, BLOCK_LEN, blocks(R)) for R in FACTORS for C in CHANNELS]
    return out + [(R, 32, SHORT_LEN, 1) for R in FACTORS]


def child(side, json_path, steps, log2):
    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H = rtlws.hip_lib()
    stream = rtlws.torch_stream_handle()
    F = rtlws.fm_lib()
    if side == "composition":
        assert F.rtlws_fm_prepare(eng.h) == 0, rtlws.fm_last_error()
    torch.manual_seed(1)
    srcs = [torch.randint(0, 256, (1 << log2, 2), dtype=torch.uint8, device=dev) for _ in range(3)]
    e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()
    rng = np.random.default_rng(1)
    plans, result = {}, {}
    for R, C, L, nb in cells(log2):
        if R not in plans:
            taps = rtlws.ddcfir_design(R, 8 * R)
            plans[R] = {"fused": lambda: rtlws.FmFirPlan.open(eng, R, taps), "composition": lambda: rtlws.DdcFirPlan.open(eng, R, taps),
                        "unfiltered": lambda: rtlws.FmBankPlan.open(eng)}[side]()
        plan = plans[R]
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
                plan.run(src, L, nb, words, st_in.data_ptr(), s, a, out_shift=SHIFT, audio_stride=n, stream=stream)
            elif side == "unfiltered":
                plan.run(R, src, L, nb, words, st_in.data_ptr(), s, a, audio_stride=n, stream=stream)
            else:
                d = inter[i % 2].data_ptr()
                plan.run(src, dec_len, words, d, out_shift=SHIFT, stream=stream)
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
    for plan in plans.values():
        plan.close()
    eng.close()
    with open(json_path, "w") as f:
        json.dump(result, f)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], args[2], int(args[3]), int(args[4]))
    log2, out_path, steps = 27, os.path.join(ROOT, "profiles", "fmfir_rates.txt"), 20
    while args:
        if args[0] == "--samples":
            log2 = int(args[1])
        elif args[0] == "--out":
            out_path = args[1]
        else:
            raise SystemExit(__doc__)
        args = args[2:]

    def run(side, nsteps):
        with tempfile.NamedTemporaryFile(suffix=".json") as tf:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, tf.name, str(nsteps), str(log2)], check=True,
                           timeout=300)
            return json.load(open(tf.name))

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("%d cmplx_u8 samples on the device, blocks of %d decimated samples, L = 8 R designed taps, out_shift %d; fused = one "
        "rtlws_fmfir_run, composition = one rtlws_ddcfir_run + C x rtlws_fm_audio_blocks, unfiltered = one rtlws_fmbank_run; a "
        "process per side and round, alternating, %d launches per round on rotating buffer sets, device events"
        % (1 << log2, BLOCK_LEN, SHIFT, steps))
    say("expected before the run: composition / fused on either side of 1 at C = 32, well above 1 on the short call")
    first = {side: run(side, 0) for side in SIDES}
    for key in first["fused"]:
        assert first["fused"][key]["digest"] == first["composition"][key]["digest"], "audio or states differ at " + key
    say("audio and states of fused and composition: equal checksums in all %d cells, compared before timing" % len(first["fused"]))
    times = {side: {} for side in SIDES}
    for _ in range(3):
        for side in SIDES:
            for key, v in run(side, steps).items():
                assert v["digest"] == first[side][key]["digest"], key
                times[side].setdefault(key, []).append(v["us"])
    for R, C, L, nb in cells(log2):
        key = "%d,%d,%d,%d" % (R, C, L, nb)
        f, c, u = times["fused"][key], times["composition"][key], times["unfiltered"][key]
        verdict = "confirmed" if max(f) < min(c) else "refuted"
        say("R=%-2d L=%-3d C=%-2d %5d x %5d  fused %8.1f .. %8.1f us (%s)  composition %8.1f .. %8.1f us (%s)  composition / fused "
            "= %.2f (medians); fused range wholly below: %s; unfiltered %8.1f .. %8.1f us, fused / unfiltered = %.2f (medians)"
            % (R, 8 * R, C, nb, L, min(f), max(f), " ".join("%.1f" % x for x in f), min(c), max(c), " ".join("%.1f" % x for x in c),
               float(np.median(c) / np.median(f)), verdict, min(u), max(u), float(np.median(f) / np.median(u))))
    say("not measured: hardware counters; odd R or L (the 2-byte load form; R = 10 takes the 4-byte one)")
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
