"""Shared by tests/test_fm_cpu.py and tests/test_fm_gpu.py: the oracle's per-block FM chain as a loop, the test
inputs, and the fused kernel's stream maps (rtl-ws_amd/csrc/fm_chain.hip) restated in numpy."""
import numpy as np

STATE = 21


def oracle_chain(oracle, iq, block_len, state, run_stage2=True):
    """nblocks calls of oracle.audio_block (= audio_fm_demodulator) -> (audio, state out).  run_stage2=False is
    src/audio_main.c:137's exhausted pool: the second half-band never ran, its delay line keeps its value."""
    iq = np.ascontiguousarray(iq, dtype=np.int32).reshape(-1, 2)
    st = np.array(state, dtype=np.float32)
    out = []
    for b in range(iq.shape[0] // block_len):
        keep = st[11:21].copy()
        a = oracle.audio_block(iq[b * block_len:(b + 1) * block_len], st)
        if run_stage2:
            out.append(a)
        else:
            st[11:21] = keep
    audio = np.concatenate(out) if out else np.zeros(0, dtype=np.float32)
    return audio, st


def random_state(seed):
    """A non-zero carried state: a phase in (-pi, pi), delay lines of limiter-sized values."""
    rng = np.random.default_rng(seed)
    st = rng.uniform(-1.0, 1.0, STATE).astype(np.float32)
    st[0] = np.float32(rng.uniform(-3.0, 3.0))
    return st


def input_a(n, seed):
    """Random int32 in +-3000 with 1 % zeros in each component: the limiter and the x == 0 branches."""
    rng = np.random.default_rng(seed)
    iq = rng.integers(-3000, 3001, size=(n, 2), dtype=np.int32)
    iq[rng.random(n) < 0.01, 0] = 0
    iq[rng.random(n) < 0.01, 1] = 0
    return iq


def input_b(n, seed):
    """A phasor of amplitude 1000 with phase steps uniform in +-1.2 rad: both sides of the limiter."""
    rng = np.random.default_rng(seed)
    ph = np.cumsum(rng.uniform(-1.2, 1.2, n))
    return np.stack([np.round(1000 * np.cos(ph)), np.round(1000 * np.sin(ph))], axis=1).astype(np.int32)


# ---- the maps of fm_chain.hip ---------------------------------------------------------------------------------

def halfband_f32(x, hist):
    """Continuous 11-tap half-band over the stream x with hist = x[-10..-1]: float32, multiply then add, the
    centre tap first and the even taps in the order of src/resample.c:57-64."""
    h0, h2, h4, h5 = np.float32(0.01824), np.float32(-0.11614), np.float32(0.34790), np.float32(0.5)
    n = x.size // 2
    z = np.concatenate([np.asarray(hist, np.float32), np.asarray(x, np.float32)])
    c = 10 + 2 * np.arange(n)
    acc = h5 * z[c - 5]
    for h, k in ((h0, 0), (h2, 2), (h4, 4), (h4, 6), (h2, 8), (h0, 10)):
        acc = acc + h * z[c - k]
    assert acc.dtype == np.float32
    return acc


def s1_to_g(s1, L):
    half = L // 2
    return (s1 // (2 * half)) * L + s1 % (2 * half)


def s2_to_w(s2, L):
    half = L // 2
    quarter = half // 2
    return (s2 // (2 * quarter)) * half + s2 % (2 * quarter)


def chain_by_maps(oracle, iq, L, state):
    """The chain as ONE continuous filter over concatenated, truncated streams -> (audio, state out)."""
    iq = np.ascontiguousarray(iq, dtype=np.int32).reshape(-1, 2)
    nb = iq.shape[0] // L
    half = L // 2
    quarter = half // 2
    demod, last_phase = oracle.fm_demod(iq, prev_phase=float(state[0]))       # limit(phase[g] - phase[g-1])
    stage1 = demod[s1_to_g(np.arange(nb * 2 * half), L)]
    work = halfband_f32(stage1, state[1:11])
    stage2 = work[s2_to_w(np.arange(nb * 2 * quarter), L)]
    audio = halfband_f32(stage2, state[11:21])
    out = np.empty(STATE, dtype=np.float32)
    out[0] = np.float32(last_phase)
    out[1:11] = np.concatenate([state[1:11], stage1])[-10:]
    out[11:21] = np.concatenate([state[11:21], stage2])[-10:]
    return audio, out


def tile_range(t, L, nb, tile):
    """tile_range() of fm_chain.hip: what tile t reads of each stream -> (n2, n1, np)."""
    quarter = (L // 2) // 2
    total = nb * quarter
    a0 = t * tile
    na = min(tile, total - a0)
    s2lo, s2hi = 2 * a0 - 10, 2 * (a0 + na - 1)
    wlo, whi = s2_to_w(max(s2lo, 0), L), s2_to_w(s2hi, L)
    s1lo = 2 * wlo - 10
    glo, ghi = s1_to_g(max(s1lo, 0), L), s1_to_g(2 * whi, L)
    return s2hi - s2lo + 1, 2 * (whi - wlo) + 11, ghi - glo + 2
