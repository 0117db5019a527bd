"""A model of the polyphase family's launch tables: which template instantiation a plan and a run launch.

Restated from rtl-ws_amd/csrc (no GPU, no build needed):
  pfb_plan.h ...... Log2Ms = 4 .. 10, Bools
  pfb_bank.hip .... with_kernel:        pfb_kernel<log2 M>
  pfbspec.hip ..... with_kernel:        pfbspec_kernel<log2 M>          (K >= F or not is a branch at run time)
  pfbxc.hip ....... with_kernel:        pfbxc_kernel<log2 M, A>, A = 2 .. 4   (the same branch at run time)
  pfbbf.hip ....... with_kernel:        pfbbf_kernel<log2 M, B>, B = 1 .. 4   (A = 1 .. 8 is a loop at run time)
                    with_power_kernel:  pfbbf_power_kernel<log2 M, B, WHOLE>
  pfbsk.hip ....... with_kernel:        pfbsk_kernel<log2 M, WHOLE>
  pfb_bank.h ...... tile_frames; the host's rule WHOLE = k_avg >= tile_frames(log2 M)

CASES holds one case per instantiation, 133 in all.  tests/test_pfb_family_matrix_cpu.py holds the model to the five
libraries' code objects both ways, tests/test_pfb_family_matrix_gpu.py launches every case.

A case fixes the library, log2 M, T (the first T that pfb_ref.SHAPES lists for that log2 M), A and B where they apply,
and K for the kernels that have WHOLE as a template parameter (K = 0: the beamformer's voltage mode, the channelizer,
and the spectrometer and the correlator, which take both of run_ks(case) through their one instantiation).  The
beamformer's A cycles through 1 .. 8 so that every A meets every B, and 5, 6 and 7 -- which no earlier suite ran --
each meet every B both where a thread has one channel (log2 M <= 8) and where it has M / 256 (log2 M >= 9)."""
from collections import namedtuple

import pfb_ksum_cases as ksum
import pfb_ref

LOG2_MS = tuple(range(4, 11))                                 # pfb_plan.h: Log2Ms
XC_INPUTS = (2, 3, 4)                                         # pfbxc.hip: Inputs
BEAMS = (1, 2, 3, 4)                                          # pfbbf.hip: Beams
MAX_BF_INPUTS = 8                                             # pfbbf.h: BfParams::src[8]
LIBRARIES = ("pfb", "pfbspec", "pfbxc", "pfbbf", "pfbsk")
# the kernels of each library, as its code object names them
KERNELS = {"pfb": ("pfb_kernel",), "pfbspec": ("pfbspec_kernel",), "pfbxc": ("pfbxc_kernel",),
           "pfbbf": ("pfbbf_kernel", "pfbbf_power_kernel"), "pfbsk": ("pfbsk_kernel",)}
COUNTS = {"pfb": 7, "pfbspec": 7, "pfbxc": 21, "pfbbf": 84, "pfbsk": 14}

TAPS_PER_BRANCH = {}
for _k, _T in pfb_ref.SHAPES:
    TAPS_PER_BRANCH.setdefault(_k, _T)
assert sorted(TAPS_PER_BRANCH) == list(LOG2_MS)


def tile_frames(k):
    """pfb_bank.h"""
    return 4096 >> k


def whole(k, k_avg):
    """launch_pfbbf_power, launch_pfbsk: the host's choice of WHOLE"""
    return k_avg >= tile_frames(k)


def sum_k(k, want_whole):
    """The K a sum kernel is launched with.  WHOLE: F + 17, several tile iterations and the last one ending inside a
    slice.  Not WHOLE: 17 where the tile then still holds two spectra (F > 34), else 3: a ragged slice either way."""
    F = tile_frames(k)
    K = F + 17 if want_whole else 17 if F > 34 else 3
    c = ksum.classify(k, K)
    if want_whole:
        assert c[0] == "K >= F" and c[1] != "1 iteration", (k, K, c)
        assert c[2] in ("last iteration shorter than a slice", "last iteration several slices, ragged"), (k, K, c)
    else:
        assert c[0] == "K < F" and c[3] == "ragged slice" and c[2] == ("several slices" if K == 17 else "one slice"), (k, K, c)
        assert K != 17 or c[1] == "G > 1", (k, K, c)
    assert whole(k, K) == want_whole
    return K


class Case(namedtuple("Case", "lib k T A B K")):
    """lib: one of LIBRARIES; A: captures (1 where the library takes one); B: beams (0 outside the beamformer); K: see
    the module's text."""

    def label(self):
        s = "%s M=%d T=%d" % (self.lib, 1 << self.k, self.T)
        if self.lib in ("pfbxc", "pfbbf"):
            s += " A=%d" % self.A
        if self.lib == "pfbbf":
            s += " B=%d %s" % (self.B, "power" if self.K else "voltage")
        if self.K:
            s += " K=%d" % self.K
        return s


def instantiation(c):
    """(kernel name, template arguments) of the instantiation case c launches, as the demangled name in the code
    object spells it: pfbbf_power_kernel<7, 3, true> -> ("pfbbf_power_kernel", (7, 3, True))."""
    assert c.lib in LIBRARIES and c.k in LOG2_MS
    if c.lib == "pfb":
        return ("pfb_kernel", (c.k,))
    if c.lib == "pfbspec":
        return ("pfbspec_kernel", (c.k,))
    if c.lib == "pfbxc":
        assert c.A in XC_INPUTS
        return ("pfbxc_kernel", (c.k, c.A))
    if c.lib == "pfbsk":
        assert c.K >= 1
        return ("pfbsk_kernel", (c.k, whole(c.k, c.K)))
    assert c.B in BEAMS and 1 <= c.A <= MAX_BF_INPUTS
    if c.K == 0:
        return ("pfbbf_kernel", (c.k, c.B))
    return ("pfbbf_power_kernel", (c.k, c.B, whole(c.k, c.K)))


def run_ks(c):
    """The K of every run of case c: the case's own, or one of each path for a kernel that chooses at run time."""
    if c.lib in ("pfbspec", "pfbxc"):
        return (sum_k(c.k, False), sum_k(c.k, True))
    return (c.K,) if c.K else ()


def bf_inputs(B, i):
    """A of the beamformer's i-th case of B beams (its 21 cases by log2 M, for each the voltage kernel, the power
    kernel for K < F and for K >= F).  Cases 0 .. 14 (log2 M <= 8) pass through every A; cases 15 .. 20 (log2 M >= 9)
    begin at A = B + 1 <= 5 and so pass through 5, 6 and 7."""
    return 1 + (i + B + 1) % MAX_BF_INPUTS


def _build():
    cases = []
    for k in LOG2_MS:
        T = TAPS_PER_BRANCH[k]
        cases.append(Case("pfb", k, T, 1, 0, 0))
        cases.append(Case("pfbspec", k, T, 1, 0, 0))
        cases += [Case("pfbxc", k, T, A, 0, 0) for A in XC_INPUTS]
        cases += [Case("pfbsk", k, T, 1, 0, sum_k(k, w)) for w in (False, True)]
    for B in BEAMS:
        i = 0
        for k in LOG2_MS:
            for K in (0, sum_k(k, False), sum_k(k, True)):
                cases.append(Case("pfbbf", k, TAPS_PER_BRANCH[k], bf_inputs(B, i), B, K))
                i += 1
    return cases


CASES = _build()


def by_library(lib):
    return [c for c in CASES if c.lib == lib]


def spell(t):
    """("pfbbf_power_kernel", (7, 3, True)) -> "pfbbf_power_kernel<7, 3, true>" """
    return "%s<%s>" % (t[0], ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in t[1]))


# The instantiations that no test and no smoke() case launched before this matrix, read once from the parametrisations
# of tests/test_pfbbf_gpu.py, test_pfbxc_gpu.py, test_pfb_ksum_gpu.py, test_pfb_family_digest_gpu.py and smoke():
#   B = 3: no plan with three beams was opened anywhere, 7 voltage and 14 power kernels;
#   B = 2 ran at log2 M 4, 6, 10 (test_pfbbf_gpu.py), 4, 8, 10 (the digests) and 5 with K = 3 (the stride test, smoke());
#   B = 4 ran everywhere (the K-sum suite takes the voltage kernel's time-major download as its reference);
#   the correlator's A = 4 ran at log2 M 4, 6, 10.
# Every channelizer, spectrometer, kurtosis and B = 1 kernel had been launched.  Committed as data: it is the record of
# what the matrix closed, and tests/test_pfb_family_matrix_cpu.py holds it to the model.
FIRST_LAUNCHED_HERE = (
    ("pfbbf_kernel", (4, 3)), ("pfbbf_kernel", (5, 3)), ("pfbbf_kernel", (6, 3)), ("pfbbf_kernel", (7, 3)),
    ("pfbbf_kernel", (8, 3)), ("pfbbf_kernel", (9, 3)), ("pfbbf_kernel", (10, 3)),
    ("pfbbf_power_kernel", (4, 3, False)), ("pfbbf_power_kernel", (4, 3, True)),
    ("pfbbf_power_kernel", (5, 3, False)), ("pfbbf_power_kernel", (5, 3, True)),
    ("pfbbf_power_kernel", (6, 3, False)), ("pfbbf_power_kernel", (6, 3, True)),
    ("pfbbf_power_kernel", (7, 3, False)), ("pfbbf_power_kernel", (7, 3, True)),
    ("pfbbf_power_kernel", (8, 3, False)), ("pfbbf_power_kernel", (8, 3, True)),
    ("pfbbf_power_kernel", (9, 3, False)), ("pfbbf_power_kernel", (9, 3, True)),
    ("pfbbf_power_kernel", (10, 3, False)), ("pfbbf_power_kernel", (10, 3, True)),
    ("pfbbf_kernel", (7, 2)), ("pfbbf_kernel", (9, 2)),
    ("pfbbf_power_kernel", (5, 2, True)),
    ("pfbbf_power_kernel", (7, 2, False)), ("pfbbf_power_kernel", (7, 2, True)),
    ("pfbbf_power_kernel", (9, 2, False)), ("pfbbf_power_kernel", (9, 2, True)),
    ("pfbxc_kernel", (5, 4)), ("pfbxc_kernel", (7, 4)), ("pfbxc_kernel", (8, 4)), ("pfbxc_kernel", (9, 4)),
)
