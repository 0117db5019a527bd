"""The frame lengths at the index borders of include/rtlws_anylen.h as data (rtl-ws_amd/csrc/spectrum_anylen.hip;
DESIGN.md 4.11), in the style of ddc_family_channels.py, and a restatement of where pass 4 (anylen_pass_b_pow) puts
things at a given N.  tests/test_anylen_borders_cpu.py holds the list to its conditions;
tests/test_anylen_gpu.py::test_border_lengths launches every length.

Pass 4 runs M / 8192 workgroups per row, M = N1 N2 = 2^m >= 2 N - 1.  A workgroup holds the T = 8192 / N2 columns
k1 = k1_0 .. k1_0 + T - 1 of all N2 values k2, element j = k1 + N1 k2, and keeps j < N.  What depends on N:
  - the thread that owns bin N - 1 (and with it the DC slot) sits in tile ((N-1) mod N1) / T, column ((N-1) mod N1) mod T;
  - a run of T consecutive j goes to T consecutive slots (j - N/2) mod N, unless the wrap at j = N/2 falls inside it:
    (N/2) mod T != 0;
  - the last live run keeps N mod T of its T elements (all of them when that is 0);
  - a workgroup whose first column is k1_0 >= N returns whole: some tile does when N <= N1 - T.
M itself changes where 2 N - 1 passes a power of two: N = 2^(m-1) is the last length of M = 2^m, and there b's wrapped
half M - N + 1 .. M - 1 begins one element after a's last, N - 1."""
import anylen_kernels as ak
import anylen_ref
import long_kernels as lk

TILE_POINTS = 8192


def geometry(N):
    """Where pass 4 puts things at frame length N."""
    m = anylen_ref.conv_log2(N)
    N1, N2 = 1 << lk.log2_n1(m), 1 << lk.log2_n2(m)
    T = TILE_POINTS // N2
    owner = (N - 1) % N1
    return dict(m=m, N1=N1, N2=N2, T=T, tiles=N1 // T,
                owner_tile=owner // T, owner_col=owner % T,       # of bin N - 1 and the DC slot
                wrap_in_run=(N // 2) % T, wrap_cuts=(N // 2) % T != 0,
                last_run_kept=N % T,
                tile_returns=N <= N1 - T)


# m -> the inner length of M = 2^m: the owner in an inner column of an inner tile, the wrap inside a run and not at
# its last element, a last run that keeps at least two elements and not all; odd at m = 15, 17, 19, even at 16, 18, 20
INNER_N = {15: 11675, 16: 22958, 17: 46381, 18: 91928, 19: 184919, 20: 379444}
SIZES = tuple(sorted(INNER_N))

_cases = [
    (63, "M = 2^14: the second tile of pass 4 returns whole (k1_0 = 64 >= N), the owner in the last column but one"),
    (64, "M = 2^14: the last N whose second tile returns whole (N = N1 - T), the owner in the last column of tile 0"),
    (65, "M = 2^14: the first N whose second tile is live, with one element kept; the owner is its column 0"),
    (127, "M = 2^14: one below N1: the row k2 = 1 is discarded whole, the wrap cuts the first run before its last element"),
    (128, "M = 2^14: N = N1: every column keeps exactly k2 = 0"),
    (129, "M = 2^14: one above N1: column 0 alone keeps k2 = 1, and owns bin N - 1"),
    (8193, "the first length of M = 2^15 (pass A at 256 points, pass B at 128)"),
]
for _m in SIZES:
    _cases.append(((1 << (_m - 1)) - 1, "the last odd length of M = 2^%d: the wrap cuts a run before its last element, "
                   "the last run loses one element" % _m + (", n^2 passes 2^37 in the chirp table" if _m == 20 else "")))
    _cases.append((1 << (_m - 1), "M = 2 N = 2^%d, the least slack: b's wrapped half begins one element after a's last; "
                   "the owner in the last column of the last tile" % _m))
    _cases.append((INNER_N[_m], "the inner length of M = 2^%d" % _m))
CASES = tuple(sorted(_cases))
LENGTHS = tuple(N for N, _ in CASES)
POW2 = tuple(N for N in LENGTHS if N >= 1 << 14 and N & (N - 1) == 0)     # those rtlws_long.h transforms too


def frames_for(N):
    """frames of a GPU case: 6 up to M = 2^17, 3 above (two rows of K = 3, one row)"""
    return 6 if anylen_ref.conv_log2(N) <= 17 else 3


def pass_b_lengths():
    """N2 -> one listed length whose pass 4 runs at N2 points: the inner length of an M = 2^m with N2 = 2^floor(m/2)"""
    return {128: INNER_N[15], 256: INNER_N[16], 512: INNER_N[18], 1024: INNER_N[20]}


def coverage_text():
    """For the documents: per convolution size what the lengths run before (anylen_kernels) and these reach."""
    lines = []
    for m in (14,) + SIZES:
        old = [N for N in list(ak.SMALL_N) + list(ak.PARITY_N.values()) if anylen_ref.conv_log2(N) == m]
        new = [N for N in LENGTHS if anylen_ref.conv_log2(N) == m]
        g = geometry(new[0])
        show = lambda ns: ", ".join("%d (tile %d col %d%s)" % (N, geometry(N)["owner_tile"], geometry(N)["owner_col"],
                                                              ", cut" if geometry(N)["wrap_cuts"] else "") for N in ns)
        lines.append("  M = 2^%d, N1 = %d, T = %d, %d tiles: before %s; new %s" % (m, g["N1"], g["T"], g["tiles"], show(old), show(new)))
    return "\n".join(lines)
