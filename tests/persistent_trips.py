"""Batch shapes that take every persistent kernel past its grid cap (no GPU, no build needed).

The hot-path kernels launch a capped grid and loop: `for (g = blockIdx.x; g < ngroups; g += gridDim.x)`.  What is
fragile sits in the second and later trips of that loop (the prefetch across the row border, the raw-buffer toggle,
the reuse of an LDS slice, the last trip's "no successor" branch), so a test has to run a batch longer than the grid,
and has to be able to tell which row a workgroup fetched.  This module holds the arithmetic for both:

  rows_for / pool_map ........ the strided spectrum kernels (spectra_fused, spectra_fused_v2, spectra_f64_fused,
                               spectra_f64_1024x at one wavefront per workgroup)
  x8_rows_for / x8_pool_map .. spectra_f64_1024x at eight wavefronts per workgroup (rows dealt through an LDS counter)
  cic_launch / cic_len ....... cicr_kernel<0|10|12>, restated from launch_cic_block_sums (resample_kernels.hip)
  stride_len ................. cic8_kernel, fm_demod_kernel, halfband_kernel (grid-stride loops, cus * 8 workgroups of 256)

spectra_direct and spectra_f64 launch one workgroup per row: they have no second trip and are left out.
tests/test_persistent_trips_cpu.py holds this module to its own conditions, tests/test_kernel_matrix_gpu.py,
tests/test_resample_gpu.py and tests/test_audio_gpu.py run the shapes.
"""
from collections import namedtuple

import kernel_matrix as km

PERSISTENT = ("spectra_fused", "spectra_fused_v2", "spectra_f64_fused", "spectra_f64_1024x")
X_STATIC_ROWS = 8                 # spectrum_f64_1024x.hip, WAVES = 8: rows dealt statically, the rest through the counter


def persistent(c):
    return km.instantiation(c)[0] in PERSISTENT


CASES = [c for c in km.CASES if persistent(c)]
FAMILIES = sorted({km.family(c) for c in CASES})


def is_x8(c):
    """spectra_f64_1024x<..., WAVES = 8>: which wavefront takes which row is not fixed."""
    name, args = km.instantiation(c)
    return name == "spectra_f64_1024x" and args[3] == 8


def pin_option(c):
    """The engine option that pins the case's grid at one workgroup per CU (shim.hip plan_f32 / plan_f64)."""
    return ("f64_blocks_per_cu" if c.f64 else "blocks_per_cu", 1)


# ---- strided spectrum kernels ---------------------------------------------------------------------------------

def rows_for(blocks):
    """The first 19 workgroups run three trips, the rest two: the batch ends ragged."""
    return 2 * blocks + 19


def _neighbours(g, blocks, rows):
    """For h = g + blocks, the row workgroup g % blocks takes after g: the rows h must not be mistaken for.  g (a stale
    or re-read frame), g + 1 (the next row in memory, not the next of this workgroup), h - 1 and h + 1 (off by one
    row).  With one workgroup g + 1 IS h: a row cannot differ from itself, so h is not its own neighbour."""
    h = g + blocks
    return [r for r in (g, g + 1, h - 1, h + 1) if r != h and 0 <= r < rows]


def check_pool_map(pm, blocks, rows, P):
    assert len(pm) == rows and all(0 <= e < P for e in pm)
    for g in range(rows - blocks):
        for r in _neighbours(g, blocks, rows):
            assert pm[g + blocks] != pm[r], (blocks, rows, g, r)


def pool_map(blocks, rows, P=4):
    """pm[g]: which of P distinct pool row groups output row g is a copy of, so that a workgroup that fetches a wrong
    row for its next trip produces a row that differs from the pool's (check_pool_map's conditions hold)."""
    assert blocks >= 1 and rows >= 1 and P >= 4
    if P == 4 and blocks % 4 == 0:
        pm = [(g + 2 * (g // blocks)) % 4 for g in range(rows)]
    else:
        # row by row, the lowest entry that differs from the rows already placed that it must differ from: at most
        # three of them (r - blocks, r - blocks + 1, r - 1), so four entries always suffice
        pm = []
        for r in range(rows):
            taken = {pm[q] for q in (r - blocks, r - blocks + 1, r - 1) if 0 <= q < r}
            pm.append(min(e for e in range(P) if e not in taken))
    check_pool_map(pm, blocks, rows, P)
    return pm


# ---- spectra_f64_1024x at eight wavefronts per workgroup ----------------------------------------------------------

def x8_rows_for(blocks):
    """Every workgroup goes past its eight statically dealt rows (nine rows each, ten for the first 19)."""
    return (X_STATIC_ROWS + 1) * blocks + 19


def x8_pool_size(blocks, rows):
    """The rows of one workgroup, b + i * blocks: the most any workgroup has."""
    return -(-rows // blocks)


def x8_pool_map(blocks, rows):
    """(pm, P): all rows of one workgroup carry pairwise different entries, whichever wavefront takes which; rows next
    to each other in memory differ too."""
    P = max(x8_pool_size(blocks, rows), 4)
    pm = [(g % blocks + g // blocks) % P for g in range(rows)]
    for b in range(min(blocks, rows)):
        own = pm[b::blocks]
        assert len(set(own)) == len(own), (blocks, rows, b)
    return pm, P


# ---- the stand-alone capped kernels -------------------------------------------------------------------------------

CicLaunch = namedtuple("CicLaunch", "chunk slice G rounds cap blocks")


def cic_launch(R, n, cus):
    """launch_cic_block_sums for R != 8: bytes of a piece (64 outputs), LDS bytes per wavefront, pieces per round,
    rounds of the launch, the cap on workgroups, workgroups (four wavefronts each, one round per wavefront and trip)."""
    assert 1 <= R <= 128 and R != 8 and n >= 1 and cus >= 1
    chunk = 128 * R
    slice_ = 16384 if chunk > 8192 else 8192
    G = slice_ // chunk
    rounds = (n // 64 + G - 1) // G
    cap = cus * (4 if slice_ == 8192 else 2)
    blocks = max(1, min((rounds + 3) // 4, cap))
    return CicLaunch(chunk, slice_, G, rounds, cap, blocks)


def cic_wave_rounds(R, n, cus):
    """Rounds each wavefront of the launch runs (cicr_kernel's loop: p0 = wave * G, += waves * G, while < pieces)."""
    L = cic_launch(R, n, cus)
    waves, pieces = 4 * L.blocks, n // 64
    return [len(range(w * L.G, pieces, waves * L.G)) for w in range(waves)]


def cic_len(R, cus):
    """The smallest length with 2 * 4 * cap + 7 full rounds (every wavefront reuses its slice once, seven reuse it
    twice), then a round of fewer than G pieces where G > 1, then 37 outputs that fill no piece."""
    L = cic_launch(R, 64, cus)
    pieces = (2 * 4 * L.cap + 7) * L.G + (1 if L.G > 1 else 0)
    return pieces * 64 + 37


def stride_len(cus):
    """cic8_kernel, fm_demod_kernel, halfband_kernel (cus * 8 workgroups of 256 threads): two whole trips, then a
    ragged third."""
    return 2 * cus * 8 * 256 + 256 * 5 + 37
