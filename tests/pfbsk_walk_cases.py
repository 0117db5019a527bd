"""The geometry of pfbsk_kernel's walk over the L sub-integrations of a row as data (csrc/pfbsk.hip):
how many steps a (log2 M, K, L) takes and how full the last one is, and the L that tests/test_pfbsk_gpu.py launches at
every K of tests/pfb_ksum_cases.py so that every such walk runs.  tests/test_pfbsk_walk_cpu.py holds the list to its
own conditions.

A workgroup owns one row.  With F = 4096 / M frames in the tile it takes
  K <  F: G = floor(F / K) sub-integrations per step, ceil(L / G) steps, the last one holding L - (steps - 1) G;
  K >= F: one sub-integration per step, L steps.
In a step that is not full the items behind its last sub-integration add no frame and store +0."""
import pfb_ksum_cases as ksum

MAX_NSUB = 65535
ROWS = 3                                              # per run: q0 = j L is not 0 for two workgroups
OLD_NSUB = 3                                          # test_every_sum_geometry_to_the_bit's L, at every K of the matrix
# (log2 M, K, L) that the suite held to the bit beside that matrix, before this list existed
OLD_OUTSIDE = ((4, 16, MAX_NSUB), (5, 3, 4), (10, 2, 5))

ONE_PARTIAL_STEP = ("1 step", "last step ragged", "G > 1")


def walk(k, K, L):
    """-> (whole, G, steps, last): the kernel's own figures; last = the sub-integrations of the last step."""
    whole, G = ksum.geometry(k, K)[:2]
    steps = -(-L // G)
    return whole, G, steps, L - (steps - 1) * G


def classify(k, K, L):
    """The class of a (log2 M, K, L): a tuple of words, one for every decision the kernel takes on L."""
    assert k in ksum.LOG2_MS and 1 <= K <= ksum.MAX_K_AVG and 1 <= L <= MAX_NSUB
    _, G, steps, last = walk(k, K, L)
    words = ("%s step%s" % ((1, 2, ">= 3")[min(steps, 3) - 1], "" if steps == 1 else "s"),)
    if G > 1:
        words += ("last step full" if last == G else "last step ragged",)
    return words + ("G > 1" if G > 1 else "G = 1",)


def enumerated(k, K):
    """The L over which every class of a (log2 M, K) shows: 1 .. 3 G + 2 (test_pfbsk_walk_cpu.py says why)."""
    return range(1, 3 * ksum.geometry(k, K)[1] + 3)


def ls(k, K):
    """The L that stand for the walks of a (log2 M, K): where G > 1 the smallest L of every class, but the one
    partial step by its largest, G - 1 (every item of the tile live but the last sub-integration's): G - 1, G, G + 1,
    2 G, 2 G + 1, 3 G.  Where G = 1 the number of steps is all there is, and L = 3 is the present matrix: 1 and 2."""
    G = ksum.geometry(k, K)[1]
    if G == 1:
        return [1, 2]
    first = {}
    for L in enumerated(k, K):
        first.setdefault(classify(k, K, L), L)
    first[ONE_PARTIAL_STEP] = G - 1
    return sorted(set(first.values()))


def ks(k):
    """The K of the walk matrix: every K < F of pfb_ksum_cases.cases(k); of K >= F, where the present matrix already
    crosses every class with three steps, F and 2 F + 3 (one tile iteration, full; three, the last one ragged)."""
    F = ksum.tile_frames(k)
    return [K for K in ksum.cases(k) if K < F or K in (F, 2 * F + 3)]


def walk_cases(k):
    """Every (K, L) the GPU matrix launches at log2 M = k beside L = 3."""
    return [(K, L) for K in ks(k) for L in ls(k, K) if L != OLD_NSUB]


def old_ls(k, K):
    """The L at which the suite held a (log2 M, K) to the bit before."""
    return sorted({OLD_NSUB} | {L for kk, KK, L in OLD_OUTSIDE if (kk, KK) == (k, K)})


def frames(K, L):
    return ROWS * L * K


def coverage():
    """-> {class: [the (log2 M, K) where it occurs, those where old_ls reached it, those where ls and L = 3 do]}, over
    every K < F of the matrix."""
    out = {}
    for k in ksum.LOG2_MS:
        for K in ks(k):
            if K >= ksum.tile_frames(k):
                continue
            old = {classify(k, K, L) for L in old_ls(k, K)}
            new = {classify(k, K, L) for L in ls(k, K) + [OLD_NSUB]}
            for c in {classify(k, K, L) for L in enumerated(k, K)}:
                row = out.setdefault(c, [0, 0, 0])
                row[0] += 1
                row[1] += c in old
                row[2] += c in new
    return out


def coverage_text():
    """coverage() as lines, for the documents."""
    return "\n".join("  %-48s at %2d (log2 M, K); before at %2d, now at %2d" % ((", ".join(c),) + tuple(row))
                     for c, row in sorted(coverage().items(), key=lambda item: (item[0][-1], item[0])))
