"""The kernels of librtlws_long.so (rtl-ws_amd/csrc/spectrum_long.hip) and the GPU test that launches each, in the
style of kernel_matrix.OTHER_KERNELS.  tests/test_long_cpu.py holds the library's code objects against this table."""

IN_CU8, IN_CS32, IN_RF32 = 0, 1, 2
ROWS_F64, ROWS_F32, ROWS_U8 = 0, 1, 2
SIZES = range(14, 21)                      # log2 n_fft


def log2_n1(m):
    return (m + 1) // 2


def log2_n2(m):
    return m // 2


_PARITY = "tests/test_long_gpu.py::test_batch_parity[%d]"

# test_batch_parity[m] runs the three inputs (pass A at N1 = 2^ceil(m/2)) and the three row kinds (pass B at
# N2 = 2^floor(m/2)); the smallest m that reaches a length is named
LONG_KERNELS = {}
for _m in reversed(SIZES):
    for _in in (IN_CU8, IN_CS32, IN_RF32):
        LONG_KERNELS["long_pass_a<%d, %d>" % (log2_n1(_m), _in)] = _PARITY % _m
    for _rows in (ROWS_F64, ROWS_F32, ROWS_U8):
        LONG_KERNELS["long_pass_b<%d, %d>" % (log2_n2(_m), _rows)] = _PARITY % _m
