"""spectrum_f64_1024x.hip: the rows of a fixed input, pinned to the bit.

The front end of the K = 1 instantiations (radix-4 over the 8-bit samples + the cross-row transpose) runs on the
matrix pipe as eight v_mfma_i32_16x16x32_i8 per frame.  It is exact integer arithmetic that hands pass A the very
integers the vector-pipe form (packed int16 adds, v_permlane swaps, sign extensions) produced, so every f64 operation
downstream sees the same operands and every row is the same, bit for bit.  The SHA-256 digests below were RECORDED
FROM THE BUILD OF THE COMMIT BEFORE THAT CHANGE (vector-pipe front end in every instantiation) on an MI355X; a digest
that differs means the integer front end is not exact or the f64 instruction stream was perturbed (a contraction, an
operand order) -- find which, a tolerance is not the answer.

Input: uniform bytes from a counter hash (splitmix64 finaliser, top byte), generated on the host with integer numpy
operations only, so it is the same on every machine."""
import hashlib

import numpy as np
import pytest

from helpers import hash_bytes

# (frames, forced wavefronts per workgroup): 8 192 frames on one workgroup of eight wavefronts per CU -- the form the
# launcher picks for batches of >= 32 rows per CU -- and a 3-row batch on one-wavefront workgroups
CASES = {"w8": (8192, 8), "w1": (3, 1)}

# recorded from the parent commit's build (see above): sha256 of the C-contiguous rows
PARENT_DIGESTS = {
    ("w8", "f32"): "d02361c22e5f25fa8c66d431945ea3882cf20141d3fc8a66cc53cc90f6714e7e",
    ("w8", "f64"): "5dc51aef830bb6f86b564c1c0e32ceba5ef984cf85a4c2e8133765fe0805a408",
    ("w1", "f32"): "27d2423e8ce159ec0cb95825156dda97d04ae484dac4fcb8d80b16dfed2da836",
    ("w1", "f64"): "9ceee2ba483d8364ac8606fa68ebefca0323b0af438001985b6e351cc3d96d22",
}


def uniform_bytes_iq(frames, seed):
    """(frames, 1024, 2) uint8: byte i = top byte of splitmix64's finaliser of (seed << 40) + i + 1."""
    return hash_bytes(frames * 1024 * 2, seed).reshape(frames, 1024, 2)


def rows_digest(engine, case, rows):
    frames, waves = CASES[case]
    iq = uniform_bytes_iq(frames, seed=frames)
    with engine.option("f64_x_waves", waves):
        got = engine.spectra(iq, 1024, f64=True, rows_f32=(rows == "f32"))
    assert got.shape == (frames, 1024) and got.dtype == (np.float32 if rows == "f32" else np.float64)
    return hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()


def test_input_generator_is_uniform_and_fixed():
    iq = uniform_bytes_iq(3, seed=3)
    assert hashlib.sha256(iq.tobytes()).hexdigest() == "aaa2f09e61ca5c1874997909e66ad0f8247b14aaf30a019932ebfac4ba33f439"
    counts = np.bincount(uniform_bytes_iq(64, seed=64).ravel(), minlength=256)
    assert counts.min() > 0 and abs(counts - 512.0).max() < 6 * np.sqrt(512.0)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["f32", "f64"])
@pytest.mark.parametrize("case", ["w8", "w1"])
def test_rows_bit_identical_to_vector_front_end(engine, case, rows):
    assert engine.get_option("f64_x1024") == 1
    assert rows_digest(engine, case, rows) == PARENT_DIGESTS[(case, rows)]
