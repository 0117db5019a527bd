"""spectrum_f64_1024x.hip: the structure of the headline kernel's frame loop, read from its gfx950 assembly.

hipcc cross-compiles without a GPU, so what tests/test_f64_1024x_digest_gpu.py pins on the device (the f64 instruction
stream of a frame) is checked here first, and with it what the frame loop and the head of a launch must NOT hold:
wave-uniform address arithmetic on the vector pipe, the atomic optimiser's wrapper around the row counter, a wait for
the first frame's samples in front of the table loads.

The frame loop of a kernel = every basic block on a cycle through the row's stores (the compiler lays the row counter's
blocks out behind the loop's exit branch, so the range runs from the first block a branch behind the last store jumps
back to, to the kernel's last label).  Instruction counts are per wavefront and frame, by mnemonic without the encoding
suffix (_e32 / _e64)."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "rtl-ws_amd")
KERNEL = "_ZN5rtlws17spectra_f64_1024xILi%dELb%dELb%dELi%dEEEvNS_16SpectraParamsF64E"      # <OUT, KONE, ROWF32, WAVES>
HEADLINE = {8: KERNEL % (0, 1, 1, 8), 1: KERNEL % (0, 1, 1, 1)}

# the f64 stream of one frame (pinned to the bit on the device), its conversions and the matrix-pipe front end
PINNED = {"v_fma_f64": 168, "v_fmac_f64": 120, "v_add_f64": 100, "v_mul_f64": 48, "v_cvt_f64_i32": 32, "v_cvt_f32_f64": 16}
MFMAS = 8
MFMA_OPERANDS = ("v_perm_b32", "v_xor_b32")       # 8 + 8: the operands of the MFMAs, they stay
# other_vector_instructions() of the frame loop at commit fe173f0 (the parent of the change that introduced this test),
# counted with this file's functions from that tree's assembly: {WAVES: count}
PARENT_OTHERS = {8: 26, 1: 10}


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def makefile_hipflags():
    text = open(os.path.join(AMD, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(assembly by kernel symbol: list of instructions and labels, resource remarks by kernel symbol)"""
    cc = hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "spectrum_f64_1024x.s"
    r = subprocess.run([cc] + makefile_hipflags() + ["-I../include", "-Icsrc", "-S", "--cuda-device-only",
                                                     "-Rpass-analysis=kernel-resource-usage",
                                                     "csrc/spectrum_f64_1024x.hip", "-o", str(out)],
                       cwd=AMD, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return parse_kernels(open(out).read()), parse_remarks(r.stderr)


def parse_kernels(text):
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_ZN5rtlws17spectra_f64_1024x\w+):", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s and not s.startswith(".") or s.endswith(":"):
            cur.append(s)
    return kernels


def parse_remarks(stderr):
    """{kernel symbol: {remark name: integer}} from -Rpass-analysis=kernel-resource-usage"""
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark:\s*(.+?):\s*(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = res.setdefault(val, {})
        elif cur is not None and re.fullmatch(r"-?\d+", val):
            cur[key] = int(val)
    return res


def mnemonic(ins):
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", ins.split()[0])


def frame_loop(ins):
    """[start, end) of the frame loop in a kernel's instruction list"""
    last_store = [i for i, s in enumerate(ins) if s.startswith("global_store_")][-1]
    labels = {s[:-1]: i for i, s in enumerate(ins) if s.endswith(":")}
    end = max(labels.values())
    assert end > last_store, "the exit label follows the loop"
    back = []
    for j in range(last_store, end):
        m = re.match(r"s_c?branch\w*\s+(\S+)", ins[j])
        if m and labels.get(m.group(1), end) < last_store:
            back.append(labels[m.group(1)])
    assert back, "no branch back over the row's stores"
    return min(back), end


def loop_body(ins):
    a, b = frame_loop(ins)
    return [s for s in ins[a:b] if not s.endswith(":")]


def vector_counts(body):
    return collections.Counter(mnemonic(s) for s in body if s.startswith("v_"))


def other_vector_instructions(body):
    """vector instructions of the loop that are not the pinned stream, the MFMAs or the MFMAs' operand preparation"""
    c = vector_counts(body)
    return {op: n for op, n in c.items() if op not in PINNED and op not in MFMA_OPERANDS and "mfma" not in op}


@pytest.mark.parametrize("waves", [8, 1])
def test_pinned_f64_stream(compiled, waves):
    c = vector_counts(loop_body(compiled[0][HEADLINE[waves]]))
    assert {op: c.get(op, 0) for op in PINNED} == PINNED
    assert sum(n for op, n in c.items() if "mfma" in op) == MFMAS
    assert c.get("v_mfma_i32_16x16x32_i8", 0) == MFMAS


@pytest.mark.parametrize("waves", [8, 1])
def test_uniform_values_stay_off_the_vector_pipe(compiled, waves):
    body = loop_body(compiled[0][HEADLINE[waves]])
    c = vector_counts(body)
    bad = [op for op in c if op in ("v_lshl_add_u64", "v_lshlrev_b64") or re.fullmatch(r"v_cmpx?_\w+_[iu]64", op)
           or op.startswith("v_mbcnt_")]
    assert not bad, bad
    loads = [s for s in body if s.startswith("global_load_ushort")]
    stores = [s for s in body if s.startswith("global_store_dword ")]
    assert len(loads) == 16 and len(stores) == 16
    for s in loads:            # global_load_ushort vdst, voffset, s[base:base+1] offset:imm
        assert re.match(r"global_load_ushort v\d+, v\d+, s\[\d+:\d+\]", s), s
    for s in stores:           # global_store_dword voffset, vdata, s[base:base+1] offset:imm
        assert re.match(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\]", s), s
    for s in loads + stores:
        m = re.search(r"offset:(-?\d+)", s)
        assert m is None or 0 <= int(m.group(1)) < 4096, s


@pytest.mark.parametrize("waves", [8, 1])
def test_one_round_trip_in_the_head(compiled, waves):
    """no wait for the first frame's samples before the last of the 24 table loads is issued"""
    ins = compiled[0][HEADLINE[waves]]
    head = ins[:frame_loop(ins)[0]]
    samples = [i for i, s in enumerate(head) if s.startswith("global_load_ushort")]
    tables = [i for i, s in enumerate(head) if s.startswith("global_load_dwordx4")]
    assert len(samples) == 16 and len(tables) == 24
    between = head[samples[0]:tables[-1]] if tables[-1] > samples[0] else []
    assert not [s for s in between if s.startswith("s_waitcnt") and "vmcnt" in s], between


@pytest.mark.parametrize("waves", [8, 1])
def test_fewer_other_vector_instructions_than_the_parent(compiled, waves):
    body = loop_body(compiled[0][HEADLINE[waves]])
    others = other_vector_instructions(body)
    total = sum(vector_counts(body).values())
    print("WAVES = %d: %d vector instructions per frame, %d of them neither f64 stream nor MFMA front end: %s (parent: %d)"
          % (waves, total, sum(others.values()), dict(others), PARENT_OTHERS[waves]))
    assert sum(others.values()) < PARENT_OTHERS[waves]


def test_no_instantiation_spills(compiled):
    remarks = {k: v for k, v in compiled[1].items() if "spectra_f64_1024x" in k}
    assert len(remarks) == 14 and set(remarks) == set(compiled[0])
    for name, r in remarks.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] <= 256, (name, r)
