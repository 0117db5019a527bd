#!/usr/bin/env python3
"""The FM receive chain on a device-resident capture: one launch of rtlws_fm_audio_blocks_cu8 (include/rtlws_fm.h)
against the six calls it replaces (rtlws_cic_block_sums, rtlws_fm_demod, rtlws_halfband, rtlws_copy_d2d,
rtlws_halfband, rtlws_copy_d2d on one stream).

    python tools/fm_chain_rates.py [--samples LOG2] [R ...]     rates: 2^27 cmplx_u8, R = 8 10 12, device events,
                                                                one process, three alternating rounds
    python tools/fm_chain_rates.py --profile-run [R ...]        a few fused launches only, to be run under
                                                                rocprofv3 --kernel-trace --stats -- python ...
    python tools/fm_chain_rates.py --dropin LIBDIR              wall time of audio_fm_demodulator per 19 200-sample
                                                                block with LIBDIR/librtlws_amd.so (run once per
                                                                library, alternating, to compare two builds)

The capture is one block (block_len = samples / R), so both sides compute the same floats: the audio of the two
is compared byte for byte before anything is timed."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))

HBM_PEAK = 8.0e12


def dropin(libdir, calls=2000, n=19200):
    L = C.CDLL(os.path.join(libdir, "librtlws_amd.so"))
    L.audio_fm_demodulator.argtypes = [C.c_void_p, C.c_int]
    L.audio_get_audio_payload.argtypes = [C.c_void_p, C.c_int]
    rng = np.random.default_rng(1)
    blk = rng.integers(-3000, 3000, size=(n, 2), dtype=np.int32)
    out = np.zeros(n // 4, dtype=np.float32)
    p, q = blk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    L.audio_init()
    for _ in range(50):
        L.audio_fm_demodulator(p, n)
        L.audio_get_audio_payload(q, out.nbytes)
    rounds = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(calls):
            L.audio_fm_demodulator(p, n)
            L.audio_get_audio_payload(q, out.nbytes)
        rounds.append(1e6 * (time.perf_counter() - t0) / calls)
    L.audio_close()
    print("audio_fm_demodulator %d samples, %s: %s us/call (three rounds of %d calls), audio checksum %.6f"
          % (n, libdir, " ".join("%.1f" % r for r in rounds), calls, float(np.abs(out).sum())))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--dropin":
        return dropin(args[1])
    profile_run = "--profile-run" in args
    args = [a for a in args if a != "--profile-run"]
    log2 = 27
    if args and args[0] == "--samples":
        log2, args = int(args[1]), args[2:]
    factors = [int(a) for a in args] or [8, 10, 12]

    import torch
    import rtlws
    dev = torch.device("cuda", 0)
    eng = rtlws.Engine(0)
    H, F = rtlws.hip_lib(), rtlws.fm_lib()
    assert F.rtlws_fm_prepare(eng.h) == 0, rtlws.fm_last_error()
    stream = rtlws.torch_stream_handle()
    src = torch.randint(0, 256, (1 << log2, 2), dtype=torch.uint8, device=dev)
    print("%d cmplx_u8 samples on the device, one block, algorithmic bytes = 2 R + 1 per decimated sample, "
          "HBM peak %.1f TB/s" % (1 << log2, HBM_PEAK / 1e12))
    for R in factors:
        n = ((1 << log2) // R) & ~3                      # decimated samples: one block
        half, quarter = n // 2, n // 4
        st = torch.zeros(48, dtype=torch.float32, device=dev)
        audio_f = torch.zeros(quarter, dtype=torch.float32, device=dev)
        dec = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        demod = torch.zeros(10 + n, dtype=torch.float32, device=dev)
        work = torch.zeros(10 + half, dtype=torch.float32, device=dev)
        audio_u = torch.zeros(quarter, dtype=torch.float32, device=dev)
        phase = torch.zeros(2, dtype=torch.float32, device=dev)

        def fused():
            rc = F.rtlws_fm_audio_blocks_cu8(eng.h, R, src.data_ptr(), n, 1, st.data_ptr(), st.data_ptr() + 96, 1,
                                             audio_f.data_ptr(), None, stream)
            assert rc == 0, rtlws.fm_last_error()

        def unfused():
            rc = (H.rtlws_cic_block_sums(eng.h, R, src.data_ptr(), n, dec.data_ptr(), stream) or
                  H.rtlws_fm_demod(eng.h, dec.data_ptr(), n, phase.data_ptr(), phase.data_ptr() + 4,
                                   demod.data_ptr() + 40, stream) or
                  H.rtlws_halfband(eng.h, demod.data_ptr(), work.data_ptr() + 40, half, stream) or
                  H.rtlws_copy_d2d(eng.h, demod.data_ptr(), demod.data_ptr() + 8 * half, 40, stream) or
                  H.rtlws_halfband(eng.h, work.data_ptr(), audio_u.data_ptr(), quarter, stream) or
                  H.rtlws_copy_d2d(eng.h, work.data_ptr(), work.data_ptr() + 8 * quarter, 40, stream))
            assert rc == 0, rtlws.last_error()

        if profile_run:
            for _ in range(5):
                fused()
            torch.cuda.synchronize()
            continue
        fused()
        unfused()
        torch.cuda.synchronize()
        assert torch.equal(audio_f, audio_u), "fused and unfused audio differ"
        demod[:10].zero_(), work[:10].zero_()
        e0, e1 = H.rtlws_event_create(), H.rtlws_event_create()
        steps = 20
        times = {"fused": [], "unfused": []}
        for _ in range(3):                               # alternating rounds
            for name, fn in (("fused", fused), ("unfused", unfused)):
                fn()
                H.rtlws_event_record(e0, eng.h, stream)
                for _ in range(steps):
                    fn()
                H.rtlws_event_record(e1, eng.h, stream)
                torch.cuda.synchronize()
                times[name].append(1e3 * H.rtlws_event_elapsed_ms(e0, e1) / steps)
        byts = n * (2 * R + 1)
        for name in ("fused", "unfused"):
            t = times[name]
            print("R=%-2d %-7s %8.1f .. %8.1f us/launch   %5.0f .. %5.0f GB/s algorithmic = %.2f .. %.2f of the peak   (%s)"
                  % (R, name, min(t), max(t), byts / max(t) / 1e3, byts / min(t) / 1e3,
                     byts / max(t) * 1e6 / HBM_PEAK, byts / min(t) * 1e6 / HBM_PEAK,
                     " ".join("%.1f" % x for x in t)))
        below = max(times["fused"]) < min(times["unfused"])
        print("R=%-2d unfused / fused = %.2f (medians); fused range wholly below the unfused one: %s; "
              "byte-count expectation (16 + 8 + 8 + 4 + 4 + 2 + 2 + 1 + 2 (R - 8)) / (2 R + 1) = %.2f"
              % (R, float(np.median(times["unfused"]) / np.median(times["fused"])), below,
                 (45 + 2 * (R - 8)) / (2 * R + 1)))
        H.rtlws_event_destroy(e0), H.rtlws_event_destroy(e1)
    eng.close()


if __name__ == "__main__":
    main()
