#!/usr/bin/env python3
"""The head of a launch of spectrum_f64_1024x.hip, per wavefront (diagnostic).

Needs a library built with -DRTLWS_X_STAMP (make -C rtl-ws_amd xvariant NAME=x_stamp EXTRA=-DRTLWS_X_STAMP) selected
with RTLWS_HIP_LIB: lane 0 of every wavefront overwrites the head of the last row it produced with ten 64-bit words,
{start, end (100 MHz), start, end (shader clocks), HW_ID, XCC_ID, rows, workgroup, tables in registers, first row
stored (100 MHz)} -- tools/r5_wave_timeline.py reads the first eight, this reads the 100 MHz ones: how long after its
start does a wavefront hold its 24 table quads and its first frame's samples (s_waitcnt 0 behind the loads), and when
has it issued the stores of its first row?  Eight-wavefront workgroups, 65 536 frames, f32 rows: the default line of
bench.py.

usage (GPU box): RTLWS_HIP_LIB=.../x_stamp/librtlws_hip.so python3 tools/x1024_launch_head.py [label]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rtl-ws_amd"))
import torch      # noqa: E402
import rtlws      # noqa: E402

N, FRAMES = 1024, 65536
label = sys.argv[1] if len(sys.argv) > 1 else "stamped build"
dev = torch.device("cuda", 0)
eng = rtlws.Engine(0)
stream = rtlws.torch_stream_handle()
desc = rtlws.make_desc(N, flags=rtlws.FLAG_ROWS_F32)
src = [torch.randint(0, 256, (FRAMES, N, 2), dtype=torch.uint8, device=dev) for _ in range(3)]
dst = [torch.empty((FRAMES, N), dtype=torch.float32, device=dev) for _ in range(3)]
eng.set_option("f64_x_waves", 8)


def q(x):
    return "p10 %6.2f  p50 %6.2f  p90 %6.2f  max %6.2f" % (*np.percentile(x, [10, 50, 90]), x.max())


def analyse(buf, what):
    head = buf[:, :20].cpu().numpy().copy().view(np.uint64)          # 10 words per row
    ok = ((head[:, 6] >= 1) & (head[:, 6] <= FRAMES) & (head[:, 7] < 65536) & (head[:, 0] < head[:, 1]) &
          (head[:, 4] < (1 << 32)) & (head[:, 8] >= head[:, 0]) & (head[:, 9] >= head[:, 8]) & (head[:, 9] <= head[:, 1]))
    w = head[ok].astype(np.int64)
    t0 = w[:, 0].min()
    start, tables, first, end = ((w[:, k] - t0) / 100.0 for k in (0, 8, 9, 1))
    print("%s, %s: %d wavefronts; launch %.1f us from the first start to the last end; rows per wavefront p50 %d" % (
        label, what, len(w), end.max(), np.median(w[:, 6])))
    print("  start after the launch's first start (us)  ", q(start))
    print("  start -> tables and first samples in regs  ", q(tables - start))
    print("  tables in registers -> first row stored     ", q(first - tables))
    print("  start -> first row stored                   ", q(first - start))
    print("  steady rows: (end - first row) / (rows - 1) ", q((end - first) / np.maximum(w[:, 6] - 1, 1)))


for i in range(600):      # settle the clock governor
    eng.spectra_batch_f64(desc, src[i % 3].data_ptr(), FRAMES, dst[i % 3].data_ptr(), stream=stream)
torch.cuda.synchronize()
analyse(dst[(600 - 1) % 3], "steady state (launch 600 of 600)")
time.sleep(0.05)
eng.spectra_batch_f64(desc, src[0].data_ptr(), FRAMES, dst[0].data_ptr(), stream=stream)
torch.cuda.synchronize()
analyse(dst[0], "isolated launch")
