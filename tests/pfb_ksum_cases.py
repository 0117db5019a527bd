"""The geometry of the polyphase family's K-frame sums as data (csrc/pfb_bank.h): which path of the
three kernels (pfbspec.hip, pfbxc.hip, pfbbf.hip) a (log2 M, K) takes, and the K that tests/test_pfb_ksum_gpu.py
launches so that every path runs.  tests/test_pfb_ksum_cpu.py shows that the list reaches every class that any
K = 1 .. 65536 reaches.

With F = 4096 / M frames in the tile and slices of L = min(16, F) frames a workgroup owns
  K <  F: G = floor(F / K) spectra in one tile, each summed in ceil(K / L) slices;
  K >= F: one spectrum over ceil(K / F) tile iterations, the last one holding K - (nit - 1) F frames."""
import functools

TILE_POINTS = 4096
LOG2_MS = tuple(range(4, 11))
MAX_K_AVG = 65536


def tile_frames(k):
    return TILE_POINTS >> k


def slice_frames(k):
    return min(16, tile_frames(k))


def geometry(k, K):
    """-> (whole, G, nit, nsl, last): the kernels' own figures; last = the frames of the last tile iteration."""
    F, L = tile_frames(k), slice_frames(k)
    if K >= F:
        nit = -(-K // F)
        return True, 1, nit, F // L, K - (nit - 1) * F
    return False, F // K, 1, -(-K // L), K


def classify(k, K):
    """The class of a (log2 M, K): a tuple of words, one for every decision the kernels take on it."""
    F, L = tile_frames(k), slice_frames(k)
    assert k in LOG2_MS and 1 <= K <= MAX_K_AVG
    whole, G, nit, nsl, last = geometry(k, K)
    if not whole:
        return ("K < F",
                "G > 1" if G > 1 else "G = 1",
                "several slices" if nsl > 1 else "one slice",
                "whole slices" if K % L == 0 else "ragged slice",
                "tile used up" if F % K == 0 else "frames of the tile unused")
    if last == F:
        tail = "last iteration full"
    elif last < L:
        tail = "last iteration shorter than a slice"
    elif last % L == 0:
        tail = "last iteration whole slices"
    else:
        tail = "last iteration several slices, ragged"
    return ("K >= F", "%s iteration%s" % ((1, 2, ">= 3")[min(nit, 3) - 1], "" if nit == 1 else "s"), tail)


def old_k_list(k):
    """What tests/test_pfbspec_gpu.py, test_pfbxc_gpu.py and test_pfbbf_gpu.py launch (their k_list, united)."""
    F = tile_frames(k)
    return sorted({K for K in (1, 2, 3, 6, F - 1, F, F + 1, 2 * F + 3) if K >= 1})


# K that stand for no class of their own and are launched all the same: what tools/pfb*_rates.py and the headers'
# examples run (K = 256 at M = 32 is the smallest of its class anyway)
EXTRAS = {5: (256,), 10: (16,)}
# and, at M = 16, a K of every slice count nsl = 4 .. 8 with G > 1 (K = 17 and 48 have 2 and 3): the spectrometer splits
# an item into (g, s) by a reciprocal of nsl, so every nsl that meets g > 0 is launched once
SLICE_COUNTS = {4: (64, 80, 96, 112, 128)}


@functools.lru_cache(maxsize=None)
def smallest_of_each_class(k):
    """-> {class: the smallest K of it} over every K = 1 .. 65536"""
    first = {}
    for K in range(1, MAX_K_AVG + 1):
        first.setdefault(classify(k, K), K)
    return first


def new_k_list(k):
    """The smallest K of every class that old_k_list(k) does not reach, the extras and the slice counts."""
    old = {classify(k, K) for K in old_k_list(k)}
    new = {K for c, K in smallest_of_each_class(k).items() if c not in old}
    return sorted((new | set(EXTRAS.get(k, ())) | set(SLICE_COUNTS.get(k, ()))) - set(old_k_list(k)))


def cases(k):
    """Every K the GPU matrix launches at log2 M = k.  K = 65536 has tests of its own."""
    return sorted(set(old_k_list(k)) | set(new_k_list(k)))


def spectra(k, K, grid=None):
    """Spectra per run: 2 per + 1 with per from the library's own *_grid call (grid(k, K) -> per; the spectrometer's
    by default): three workgroups where G > 1, the last one holding a single spectrum; 3 where K >= F."""
    if grid is None:
        import rtlws

        def grid(k, K):
            rc, _, _, _, per = rtlws.pfbspec_grid(k, 1, 1 << k, K, 1)
            assert rc == 0
            return per
    per = grid(k, K)
    assert per == geometry(k, K)[1]
    return 2 * per + 1


def several_spectra_several_slices(k):
    """The smallest K of the class "G > 1, several slices" (16 < K <= F / 2), or None where it does not exist."""
    for K in cases(k):
        c = classify(k, K)
        if c[:3] == ("K < F", "G > 1", "several slices"):
            return K
    return None
