"""GPU suite of include/rtlws_clean.h (librtlws_clean.so) against its numpy restatement (tests/clean_ref.py), every output
word bit for bit: out (f32 on uint32 views, NaN by place), keep, stats and nkept; NaN in both strides' padding of the
input, a preset pattern in the output's padding and behind every output.  Every row shape (G = 1, a padded tree, part of a
wavefront, both sides of the 256-channel group, the one-row workgroup; every count of lanes a row takes, 1 .. 1024, so
every depth of the zero-DM tree inside a wavefront and across one to sixteen of them; every length stage 2 sorts, 4 .. 4096,
and both sides of its 64 KiB of LDS) at every block length and run length with the filter on and off; the median's
index at one, two, all but one and all channels valid; signed rows; a static mask, non-finite samples, constant channels, an all-flagged block and the
thresholds' ends; in place; each optional output NULL; one plan many times and beside another; a run from a later block;
the three launches captured and replayed; every refusal of a run; and the chain into rtlws_dedisp_run."""

import numpy as np
import pytest

import clean_ref
import dedisp_ref

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.678)
INF = float("inf")
# the feature's own channel counts, and those that tests/search_family_matrix.py found no test at: a cross-lane tree of 1, 3
# and 5 levels (8, 20, 128), the padded row of four wavefronts (516), the rows of eight (1028, 2048), and the two sides of
# stage 2's 64 KiB of LDS (2048, 2052); between them sort lengths 8, 32, 128 and 2048
FIRST_NCHANS = (4, 12, 64, 252, 256, 260, 1024, 4096)
NCHANS, BLOCKS = tuple(sorted(FIRST_NCHANS + (8, 20, 128, 516, 1028, 2048, 2052))), (32, 33, 40, 512)
# the rows of eight and of sixteen wavefronts beside 4096: the short blocks and three run lengths, which keep a case to a
# few seconds (the restatement's time goes with rows x channels)
WIDE = (1028, 2048, 2052)
SHAPES = [(nchan, B) for B in BLOCKS for nchan in NCHANS if not (nchan in WIDE and B == 512)]


def _nrows(B, nchan=4):
    if nchan in WIDE:
        return (B, B + 1, 2 * B + B // 2)
    return (B, B + 1, 2 * B, 2 * B + B // 2, 5 * B + 7)


@pytest.fixture(scope="module")
def clean(built):
    import rtlws.clean
    return rtlws.clean


def _same_bits(got, want, what=None):
    """bit for bit, NaN by place (the default NaN of the host's arithmetic and the device's may differ)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5])
        return
    nan, gnan = np.isnan(want), np.isnan(got)
    bad = (gnan != nan) | (~nan & (np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)))
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _check(clean, engine, x, B, mask=None, t_mean=6.0, t_sigma=6.0, zerodm=True, want=("keep", "stats", "nkept"), in_place=False, name=None, ref=None):
    """x float32 [nrows, M] through rtlws.clean.clean with NaN in the input stride's padding, another output stride and
    preset guards, against the restatement (ref: its outputs where the caller has them already) -> the restatement's"""
    nrows, M = x.shape
    stride, ostride = M + 4, M + 8
    padded = np.full((nrows, stride), np.nan, np.float32)
    padded[:, :M] = x
    out, keep, stats, nkept = clean.clean(engine, padded, B, mask, t_mean, t_sigma, zerodm, want, in_stride=stride, nchan=M,
                                          out_stride=None if in_place else ostride, in_place=in_place, fill=FILL)
    ref = clean_ref.clean_ref(x, B, mask, t_mean, t_sigma, zerodm) if ref is None else ref
    nblocks = clean_ref.blocks_of(nrows, B)
    fill_bits = FILL.view(np.uint32)
    if in_place:
        assert out.shape == (nrows * stride,)
        out = out.reshape(nrows, stride)
        assert np.isnan(out[:, M:]).all(), name                                 # the padding as the caller left it
    else:
        assert out.shape == (nrows * ostride + clean.GUARD,) and np.all(out[nrows * ostride:].view(np.uint32) == fill_bits), name
        out = out[:nrows * ostride].reshape(nrows, ostride)
        assert np.all(out[:, M:].view(np.uint32) == fill_bits), name
    _same_bits(np.ascontiguousarray(out[:, :M]), ref[0], (name, "out"))
    for got, count, dtype, guard, wanted, what in ((keep, nblocks * M, np.uint8, clean.KEEP_FILL, "keep" in want, "keep"),
                                                   (stats, nblocks * M * 2, np.float32, FILL, "stats" in want, "stats"),
                                                   (nkept, nblocks, np.int32, FILL.view(np.int32), "nkept" in want, "nkept")):
        assert got.shape == (count + clean.GUARD,) and got.dtype == dtype, (name, what)
        assert np.all(got[count if wanted else 0:] == guard), (name, what)
    if "keep" in want:
        _same_bits(keep[:nblocks * M].reshape(nblocks, M), ref[1], (name, "keep"))
    if "stats" in want:
        _same_bits(stats[:nblocks * M * 2].reshape(nblocks, M, 2), ref[2], (name, "stats"))
    if "nkept" in want:
        _same_bits(nkept[:nblocks], ref[3], (name, "nkept"))
    return ref


def test_the_cases_cover_the_borders(clean):
    """G = 1, a padded tree, a part of a wavefront and a whole one, one to sixteen wavefronts a row; blocks whose residue
    classes are unequal; a last block of one row, of half a block and of seven rows"""
    assert [clean_ref.pow2_at_least(m // 4) for m in NCHANS] == [1, 2, 4, 8, 16, 32, 64, 64, 128, 256, 256, 512, 512, 1024, 1024]
    assert [clean.geometry(m, 32, 32)[2][2] for m in NCHANS] == [256] * 11 + [512, 512, 1024, 1024]
    assert [clean.geometry(m, 32, 32)[1][0] for m in NCHANS] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 8, 9, 16]
    assert [B % 8 for B in BLOCKS] == [0, 1, 0, 0] and max(_nrows(512)) <= 2600
    # what the library itself reports, class by class: the lanes a row takes (a block of 16384 rows is 1024 G / T
    # workgroups of the third launch: 16 T / G rows each), the wavefronts of a row, the keys stage 2 sorts, its threads,
    # and its LDS on both sides of 64 KiB
    lanes, waves, keys, threads, lds = [], [], [], [], []
    for m in NCHANS:
        rc, blocks, thr, bytes_, _, _, _ = clean.geometry(m, 16384, 16384)
        assert rc == 0 and (blocks[2] * thr[2]) % 1024 == 0
        G = blocks[2] * thr[2] // 1024
        assert G == clean_ref.pow2_at_least(m // 4) and bytes_[2] == (8 * thr[2] if G > 64 else 0)
        lanes.append(G)
        waves.append(max(G // 64, 1))
        keys.append((bytes_[1] - 128) // 16)
        threads.append(thr[1])
        lds.append(bytes_[1])
    assert set(lanes) == {1 << k for k in range(11)}                            # every depth of the cross-lane tree, 0 .. 6, and of the LDS tree
    assert set(waves) == {1, 2, 4, 8, 16}                                       # every entry of clean.hip's RowWaves
    assert keys == [clean_ref.pow2_at_least(m) for m in NCHANS] and set(keys) == {4 << k for k in range(11)}
    assert {(t, k // t if k > t else 1) for t, k in zip(threads, keys)} == {(64, 1), (64, 2), (128, 2), (256, 2), (512, 2), (1024, 2), (1024, 4)}
    assert [k for t, k in zip(threads, keys) if (t, k // t) == (64, 2)] == [128] and [k for t, k in zip(threads, keys) if (t, k // t) == (1024, 2)] == [2048, 2048]
    assert max(v for v in lds if v <= 65536) == lds[NCHANS.index(2048)] == 32896 and min(v for v in lds if v > 65536) == lds[NCHANS.index(2052)] == 65664
    assert all(m < 1028 or m == 4096 for m in NCHANS if m not in WIDE) and len(SHAPES) == len(NCHANS) * len(BLOCKS) - len(WIDE)


@pytest.mark.parametrize("nchan,B", SHAPES)
def test_every_row_shape_block_length_and_run_length(clean, engine, nchan, B):
    for nrows in _nrows(B, nchan):
        x = dedisp_ref.pooled_rows(nrows, nchan, seed=nchan + B + nrows)
        for zerodm in (True, False):
            _check(clean, engine, x, B, zerodm=zerodm, name=(nchan, B, nrows, zerodm))


@pytest.mark.parametrize("nchan,B", [(12, 33), (260, 40), (1024, 32)])
def test_signed_rows(clean, engine, nchan, B):
    x = dedisp_ref.signed_rows(5 * B + 7, nchan, seed=nchan)
    for zerodm in (True, False):
        ref = _check(clean, engine, x, B, zerodm=zerodm, name=("signed", nchan, zerodm))
    assert np.signbit(ref[0]).any() and 0 < ref[1].mean()


@pytest.mark.parametrize("nchan,B", [(12, 32), (260, 33), (4096, 40), (2048, 33)])
def test_special_values_and_thresholds(clean, engine, nchan, B):
    """a static mask, a NaN, an Inf and a constant channel, a block of constants (nothing kept there), at t = 0, 6 and
    +Inf in both places"""
    nrows = 3 * B + 5
    x = dedisp_ref.pooled_rows(nrows, nchan, seed=nchan + 1).copy()
    x[B + 3, 2], x[7, 9], x[:, 5] = np.nan, np.inf, 0.1
    x[2 * B:] = np.arange(nchan, dtype=np.float32)[None, :] + 0.3               # blocks 2 and 3 are constants throughout
    mask = dedisp_ref.random_mask(nchan, 3)
    mask[2] = mask[9] = mask[5] = 1
    kept = {}
    for t_mean, t_sigma in ((0.0, INF), (INF, 0.0), (6.0, 6.0), (INF, INF), (0.0, 0.0)):
        ref = _check(clean, engine, x, B, mask, t_mean, t_sigma, True, name=("special", nchan, t_mean, t_sigma))
        assert not ref[1][1, 2] and not ref[1][0, 9] and not ref[1][:, 5].any() and ref[3][2] == 0 and not ref[0][2 * B:].any()
        assert not ref[1][:, mask == 0].any()
        kept[(t_mean, t_sigma)] = ref[3][0]
    # t = 0 keeps the median's channel alone; no test keeps every valid channel (the Inf and the constant one are not)
    assert kept[(0.0, INF)] == 1 and kept[(INF, 0.0)] == 1 and kept[(0.0, 0.0)] <= 1 and kept[(INF, INF)] == mask.sum() - 2
    _check(clean, engine, x, B, mask, 6.0, 6.0, False, name=("special, unfiltered", nchan))


@pytest.mark.parametrize("nchan,B", [(4, 32), (252, 33), (1024, 40), (2048, 40)])
def test_in_place(clean, engine, nchan, B):
    x = dedisp_ref.pooled_rows(2 * B + B // 2, nchan, seed=nchan + 2)
    for zerodm in (True, False):
        _check(clean, engine, x, B, zerodm=zerodm, in_place=True, name=("in place", nchan, zerodm))


@pytest.mark.parametrize("nchan", [128, 2048])
def test_the_median_is_element_nvalid_minus_one_over_two(clean, engine, nchan):
    """a static mask that leaves 1, 2, sort_len - 1 and sort_len channels valid, where a thread of stage 2 holds two keys
    (64 threads at 128 keys, 1024 at 2048): with t = 0 in one test and +Inf in the other the block keeps the one channel
    whose mu (or sd) is element (nvalid - 1) / 2 of the valid ones in ascending order -- at nvalid 2 the smaller of the
    two, at an even nvalid the lower of the middle pair -- found here by numpy's own sort of the statistics"""
    B, nrows = 32, 33
    assert clean_ref.pow2_at_least(nchan) == nchan and clean.geometry(nchan, B, nrows)[2][1] == nchan // 2
    x = dedisp_ref.pooled_rows(nrows, nchan, seed=nchan + 3)
    order = np.random.default_rng(nchan).permutation(nchan)
    for nvalid in (1, 2, nchan - 1, nchan):
        mask = np.zeros(nchan, np.uint8)
        mask[order[:nvalid]] = 1
        for which, (t_mean, t_sigma) in enumerate(((0.0, INF), (INF, 0.0))):
            ref = _check(clean, engine, x, B, mask, t_mean, t_sigma, True, name=("median", nchan, nvalid, which))
            for b in range(2):
                j0 = clean_ref.window_start(b, B, nrows)
                mu, sd, _, _, valid = clean_ref.stats_ref(x[j0:j0 + B], mask)
                assert valid.sum() == nvalid
                stat = (mu, sd)[which]
                at = np.flatnonzero(valid)[np.argsort(stat[valid], kind="stable")]
                assert len(set(stat[valid].tolist())) == nvalid                 # no ties: one channel is the median
                assert np.flatnonzero(ref[1][b]).tolist() == [at[(nvalid - 1) // 2]] and ref[3][b] == 1, (nvalid, which, b)
        _check(clean, engine, x, B, mask, 6.0, 6.0, True, name=("median, 6 MADs", nchan, nvalid))


def test_each_optional_output_null_in_turn(clean, engine):
    x = dedisp_ref.pooled_rows(2 * 40 + 1, 260, seed=5)
    ref = clean_ref.clean_ref(x, 40, None, 6.0, 6.0, True)
    for want in (("stats", "nkept"), ("keep", "nkept"), ("keep", "stats"), ()):
        _check(clean, engine, x, 40, want=want, name=want, ref=ref)


def test_one_plan_many_runs_and_two_plans_side_by_side(clean, engine):
    """two plans of different shapes, run in turn twice over fresh buffers, the second time over other rows: every run the
    restatement's bits, and two runs over the same rows the same bits"""
    cases = []
    for nchan, B, nrows, zerodm in ((260, 33, 5 * 33 + 7, True), (64, 40, 100, False)):
        cases.append(dict(nchan=nchan, B=B, nrows=nrows, zerodm=zerodm, plan=clean.CleanPlan(engine, nchan, B, None, 6.0, 6.0, zerodm)))
    for seed in (1, 2, 2):
        held = []
        for k in cases:
            x = dedisp_ref.signed_rows(k["nrows"], k["nchan"], seed=seed + k["nchan"])
            nb = clean_ref.blocks_of(k["nrows"], k["B"])
            bufs = [engine.upload(x), engine.upload(np.full(x.size + 8, FILL, np.float32)), engine.upload(np.full(nb * k["nchan"] + 8, 0xA5, np.uint8)),
                    engine.upload(np.full(nb * k["nchan"] * 2 + 8, FILL, np.float32)), engine.upload(np.full(nb + 8, -7, np.int32))]
            k["plan"].run(bufs[0], k["nchan"], k["nrows"], bufs[1], k["nchan"], bufs[2], bufs[3], bufs[4])
            held.append((x, nb, bufs))
        engine.sync()
        for k, (x, nb, bufs) in zip(cases, held):
            want = clean_ref.clean_ref(x, k["B"], None, 6.0, 6.0, k["zerodm"])
            shapes = ((np.float32, x.size), (np.uint8, nb * k["nchan"]), (np.float32, nb * k["nchan"] * 2), (np.int32, nb))
            for buf, (dtype, count), w, guard in zip(bufs[1:], shapes, want, (FILL, 0xA5, FILL, -7)):
                got = engine.download(buf, dtype, (count + 8,))
                assert np.all(got[count:] == guard)
                _same_bits(got[:count].reshape(w.shape), w, (k["nchan"], seed))
            for buf in bufs:
                buf.free()
    for k in cases:
        k["plan"].close()


def test_a_run_from_a_later_block(clean, engine):
    """the run over the rows from 2 B on: blocks 2 .. of the whole run, bit for bit; the rows stay where they are, the
    pointer moves"""
    nchan, B, nrows, b0 = 260, 40, 5 * 40 + 7, 2
    x = dedisp_ref.signed_rows(nrows, nchan, seed=11)
    whole = clean_ref.clean_ref(x, B, None, 6.0, 6.0, True)
    plan = clean.CleanPlan(engine, nchan, B, None, 6.0, 6.0, True)
    rows, out = engine.upload(x), engine.upload(np.full(x.size, FILL, np.float32))
    nb = clean_ref.blocks_of(nrows, B) - b0
    keep, stats, nkept = engine.upload(np.zeros(nb * nchan, np.uint8)), engine.upload(np.zeros(nb * nchan * 2, np.float32)), engine.upload(np.zeros(nb, np.int32))
    plan.run(rows.ptr + b0 * B * nchan * 4, nchan, nrows - b0 * B, out.ptr + b0 * B * nchan * 4, nchan, keep, stats, nkept)
    engine.sync()
    got = engine.download(out, np.float32, x.shape)
    assert np.all(got[:b0 * B] == FILL)
    _same_bits(np.ascontiguousarray(got[b0 * B:]), whole[0][b0 * B:], "out")
    _same_bits(engine.download(keep, np.uint8, (nb, nchan)), whole[1][b0:], "keep")
    _same_bits(engine.download(stats, np.float32, (nb, nchan, 2)), whole[2][b0:], "stats")
    _same_bits(engine.download(nkept, np.int32, (nb,)), whole[3][b0:], "nkept")
    plan.close()
    for buf in (rows, out, keep, stats, nkept):
        buf.free()


def test_capture_and_replay(built, clean):
    """tests/test_fold_gpu.py::test_capture_and_replay's pattern: the capture of the three launches enqueues nothing, and a
    replay over new rows gives the restatement's bits for them"""
    import torch
    eng = built.Engine(0)
    nchan, B, nrows = 260, 40, 5 * 40 + 7
    nb = clean_ref.blocks_of(nrows, B)
    hosts = [dedisp_ref.signed_rows(nrows, nchan, seed=s) for s in (31, 32)]
    dev = torch.device("cuda", 0)
    rows = torch.from_numpy(hosts[0]).to(dev)
    outs = [torch.from_numpy(np.full(n + 8, v, t)).to(dev) for n, v, t in ((nrows * nchan, FILL, np.float32), (nb * nchan, 0xA5, np.uint8),
                                                                          (nb * nchan * 2, FILL, np.float32), (nb, -7, np.int32))]
    before = [o.clone() for o in outs]
    plan = clean.CleanPlan(eng, nchan, B, None, 6.0, 6.0, True)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan.run(rows.data_ptr(), nchan, nrows, outs[0].data_ptr(), nchan, outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                     stream=built.torch_stream_handle())
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(o, b) for o, b in zip(outs, before))                  # capture enqueued nothing
    for host in hosts:
        rows.copy_(torch.from_numpy(host))
        for o, b in zip(outs, before):
            o.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        for o, b, w in zip(outs, before, clean_ref.clean_ref(host, B, None, 6.0, 6.0, True)):
            got = o.cpu().numpy()
            assert np.array_equal(got[w.size:], b.cpu().numpy()[w.size:])
            _same_bits(got[:w.size].reshape(w.shape), w, "replayed")
    plan.close()
    eng.close()


def test_every_refusal_of_a_run(clean, engine):
    """with a live plan: each refusal of the header's list in its order, -1 and the text, and nothing written"""
    nchan, B, nrows = 8, 32, 64
    plan = clean.CleanPlan(engine, nchan, B)
    rows = engine.upload(np.zeros((nrows + 1, nchan), np.float32))
    out = engine.upload(np.full(nrows * nchan + 8, FILL, np.float32))
    side = engine.upload(np.full(64, FILL, np.float32))
    L = clean.lib()
    run = lambda d_rows, in_stride, n, d_out, out_stride, d_keep=None, d_stats=None, d_nkept=None: L.rtlws_clean_run(
        plan.h, d_rows, in_stride, n, d_out, out_stride, d_keep, d_stats, d_nkept, None)
    overlap = "d_out overlaps d_rows (in place: d_out == d_rows with equal strides)"
    for args, text in (((rows.ptr, nchan, -1, out.ptr, nchan), "nrows must be 0 .. 2^24"), ((rows.ptr, nchan, (1 << 24) + 1, out.ptr, nchan), "nrows must be 0 .. 2^24"),
                       ((rows.ptr, 0, nrows, out.ptr, nchan), "in_stride must be >= 4 and a multiple of 4"),
                       ((rows.ptr, nchan + 2, nrows, out.ptr, nchan), "in_stride must be >= 4 and a multiple of 4"),
                       ((rows.ptr, nchan, nrows, out.ptr, 2), "out_stride must be >= 4 and a multiple of 4"),
                       ((rows.ptr, nchan, nrows, out.ptr, nchan + 1), "out_stride must be >= 4 and a multiple of 4"),
                       ((None, nchan, nrows, out.ptr, nchan), "null pointer"), ((rows.ptr, nchan, nrows, None, nchan), "null pointer"),
                       ((rows.ptr + 8, nchan, nrows, out.ptr, nchan), "d_rows must be 16-byte aligned"),
                       ((rows.ptr, nchan, nrows, out.ptr + 4, nchan), "d_out must be 16-byte aligned"),
                       ((rows.ptr, nchan, nrows, out.ptr, nchan, side.ptr + 1, side.ptr + 2), "d_stats must be 4-byte aligned"),
                       ((rows.ptr, nchan, nrows, out.ptr, nchan, side.ptr + 1, side.ptr, side.ptr + 130), "d_nkept must be 4-byte aligned"),
                       ((rows.ptr, 4, nrows, out.ptr, nchan), "in_stride must be >= nchan"), ((rows.ptr, nchan, nrows, out.ptr, 4), "out_stride must be >= nchan"),
                       ((rows.ptr, nchan, B - 1, out.ptr, nchan), "nrows must be 0 or at least block_rows"),
                       ((rows.ptr, nchan, nrows, rows.ptr + 16, nchan), overlap), ((rows.ptr, nchan, nrows, rows.ptr, nchan + 4), overlap),
                       ((rows.ptr + 32, nchan, nrows, rows.ptr, nchan), overlap), ((rows.ptr, nchan, nrows, rows.ptr + (nrows * nchan - 4) * 4, nchan), overlap)
                       ):
        assert run(*args) == -1 and clean.last_error() == "rtlws_clean_run: " + text, (args, clean.last_error())
    # a plan of 4096 channels holds 1024 blocks; the refusal comes before anything is read (in place: no overlap to find first)
    wide = clean.CleanPlan(engine, 4096, B)
    assert L.rtlws_clean_run(wide.h, rows.ptr, 4096, 1024 * B + 1, rows.ptr, 4096, None, None, None, None) == -1
    assert clean.last_error() == "rtlws_clean_run: more blocks than the plan's workspace holds (clean the rows in pieces of whole blocks)"
    wide.close()
    assert run(rows.ptr, nchan, 0, out.ptr, nchan) == 0 and clean.last_error() == ""                # nrows 0 does nothing
    assert clean.geometry(nchan, B, (1 << 19) * B)[0] == 0
    engine.sync()
    assert np.all(engine.download(out, np.float32, (nrows * nchan + 8,)) == FILL) and np.all(engine.download(side, np.float32, (64,)) == FILL)
    assert not engine.download(rows, np.float32, (nrows + 1, nchan)).any()
    # d_out right behind the last element d_rows reads is no overlap
    assert run(rows.ptr, nchan, nrows, rows.ptr + nrows * nchan * 4, nchan) == 0 and clean.last_error() == ""
    engine.sync()
    plan.close()
    for buf in (rows, out, side):
        buf.free()


def test_the_chain_into_dedispersion(clean, engine):
    """a small waterfall (64 x 1500, blocks of 256) with a hot, a bursty and a dead channel, an undispersed burst and a
    dispersed pulse of 1.5 sigma per channel: the cleaned rows through rtlws_dedisp_run with no mask are dedisp_ref's bits of
    clean_ref's rows; inside every block they are the bits of the run with keep[b] as the mask; and the planted pulse is
    the series' strict maximum"""
    k = dict(nchan=64, nrows=1500, B=256, sweep=100, pulse_row=700, burst_row=400, hot=(17,), bursty=(40,), dead=3, pulse_amp=1.5)
    x, delays = clean_ref.sky(7, **k)
    out, keep, stats, nkept = clean.clean(engine, x, k["B"], None, 6.0, 6.0, True)
    want = clean_ref.clean_ref(x, k["B"], None, 6.0, 6.0, True)
    for got, w, what in zip((out, keep, stats, nkept), want, ("out", "keep", "stats", "nkept")):
        _same_bits(got, w, what)
    assert not keep[:, [17, 40, 3]].any() and keep.sum() == 6 * 61
    table = np.stack([delays, np.zeros(64, np.int32)])
    series = engine.dedisp(out, table)
    _same_bits(series, dedisp_ref.dedisp_ref(want[0], table), "series")
    for b in range(keep.shape[0]):
        part = np.ascontiguousarray(out[b * k["B"]:min((b + 1) * k["B"], k["nrows"])])
        _same_bits(engine.dedisp(part, table // 2), engine.dedisp(part, table // 2, keep[b]), ("masked", b))
        _same_bits(engine.dedisp(part, table // 2, keep[b]), dedisp_ref.dedisp_ref(part, table // 2, keep[b]), ("masked, restated", b))
    at = int(np.argmax(series[0]))
    assert at in (k["pulse_row"], k["pulse_row"] + 1) and (series[0] == series[0, at]).sum() == 1
    assert series[0, at] > 8.0 * np.sqrt(61.0) and np.abs(series[1, k["burst_row"]:k["burst_row"] + 3]).max() < 1e-3 * np.sqrt(61.0)
    assert np.array_equal(clean.union_mask(keep, 1.0), clean_ref.union_mask(want[1], 1.0)) and clean.union_mask(keep, 1.0).sum() == 61
