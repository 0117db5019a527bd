"""The kernels of librtlws_anylen.so (rtl-ws_amd/csrc/spectrum_anylen.hip) and the GPU test that launches each, in the
style of long_kernels.py.  tests/test_anylen_cpu.py holds the library's code objects against this table."""
from anylen_ref import conv_log2
from long_kernels import IN_CU8, IN_CS32, IN_RF32, ROWS_F64, ROWS_F32, ROWS_U8, log2_n1, log2_n2

# one frame length per convolution size M = 2^m above the smallest (tests/test_anylen_gpu.py::test_parity_by_conv_size)
PARITY_N = {15: 12000, 16: 16385, 17: 32769, 18: 65537, 19: 131073, 20: 262145}
# ... and M = 2^14: every N <= 8192 (test_small_and_awkward_lengths)
SMALL_N = (2, 3, 5, 1000, 1001, 2047, 8191, 8192)


_PARITY = "tests/test_anylen_gpu.py::test_parity_by_conv_size[%d]"

# test_parity_by_conv_size[N] runs the three inputs (pass 1 at N1 = 2^ceil(m/2)), the three row kinds (pass 4 at
# N2 = 2^floor(m/2)) and with them passes 2 (N2) and 3 (N1); the smallest m that reaches a length is named
ANYLEN_KERNELS = {}
for _m in sorted(PARITY_N, reverse=True):
    _t = _PARITY % PARITY_N[_m]
    for _in in (IN_CU8, IN_CS32, IN_RF32):
        ANYLEN_KERNELS["anylen_pass_a_in<%d, %d>" % (log2_n1(_m), _in)] = _t
    ANYLEN_KERNELS["anylen_pass_a_ws<%d>" % log2_n1(_m)] = _t
    ANYLEN_KERNELS["anylen_pass_b_cplx<%d>" % log2_n2(_m)] = _t
    for _rows in (ROWS_F64, ROWS_F32, ROWS_U8):
        ANYLEN_KERNELS["anylen_pass_b_pow<%d, %d>" % (log2_n2(_m), _rows)] = _t
# M = 2^14 (N1 = N2 = 128): pass 1 and pass 4 in every kind at N = 1001, passes 2 and 3 with them
_SMALL = "tests/test_anylen_gpu.py::test_small_and_awkward_lengths[1001]"
for _in in (IN_CU8, IN_CS32, IN_RF32):
    ANYLEN_KERNELS["anylen_pass_a_in<7, %d>" % _in] = _SMALL
ANYLEN_KERNELS["anylen_pass_a_ws<7>"] = _SMALL
