"""One reference, many tests on the MI355X (peaq_batch_gather, peaq_batch_run_host_refs; Python gather / run_host_refs /
run_files(share_refs=); the CLI's --list and --no-share-refs).

Yardstick for the gather: numpy indexing, and peaq_batch_cut where src is the identity.  Yardstick for the feed:
peaq_batch_run_host on the pairs written out, one (reference, test) per test -- the contract of the header.  Every
comparison is bit for bit (the FP32 samples as uint32, the bytes of the 16 doubles of a result and of a delay record, so
NaN payloads and NaN results count); there is no tolerance anywhere in this file.  Signals and helpers are those of
tests/test_gpu_pcm.py."""
import functools

import numpy as np
import pytest

import test_gpu_pcm as pcm
from test_gpu_pcm import assert_same_rows, ctx

pytestmark = pytest.mark.gpu

# ---- gather -------------------------------------------------------------------------------------------------------
ROWS, IN_STRIDE, OUT_STRIDE = 3, 1027, 1031          # odd strides: bases on every 16-byte phase, source phases apart from them
SRC = (0, 2, 0, 2, 2, 0, 2)                          # row 0 three times, row 2 four times, row 1 never
SKIPS = (0, 1, 2, 3, 5)
KEEPS = (0, 1, 3, 4, 5, 1024)
SPECIAL_BITS = (0x7FA00001, 0xFFA12345, 0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x00000001, 0x807FFFFF, 0x80000000, 0x007FFFFF)


def gather_input(channels):
    """random bit patterns; row 0, the one named three times, carries NaN payloads and denormals at its start, around
    the skips and at its end"""
    rng = np.random.default_rng(77 + channels)
    x = rng.integers(0, 1 << 32, (ROWS, IN_STRIDE, channels), dtype=np.uint64).astype(np.uint32)
    sp = np.array(SPECIAL_BITS, np.uint32)
    flat = x[0].reshape(-1)
    flat[:len(sp)] = sp
    flat[-len(sp):] = sp
    return x


def gather_cases():
    """seven outputs per call; over the calls every n_keep meets every skip (a sum beyond the row is cut to the row)"""
    for rot in range(len(KEEPS)):
        skip = np.array([SKIPS[(p + rot) % len(SKIPS)] for p in range(len(SRC))], np.uint32)
        keep = np.array([KEEPS[(2 * p + rot) % len(KEEPS)] for p in range(len(SRC))], np.uint32)
        yield skip, np.minimum(keep, IN_STRIDE - skip).astype(np.uint32)


def test_gather_cases_cover_what_they_claim():
    seen = set()
    for skip, keep in gather_cases():
        seen |= {(int(s), min(int(k), 1022)) for s, k in zip(skip, keep)}
    assert {s for s, _ in seen} == set(SKIPS) and {k for _, k in seen} == {0, 1, 3, 4, 5, 1022}
    assert {(s, 1022) for s in SKIPS} <= seen          # every source phase with a body of many vectors behind it
    assert {p * OUT_STRIDE % 4 for p in range(len(SRC))} == {0, 1, 2, 3}     # mono: every phase of the destination


@pytest.mark.parametrize("offset", [0, 1], ids=["base", "base+1"])
@pytest.mark.parametrize("channels", [1, 2])
def test_gather_equals_numpy_indexing_bit_for_bit(channels, offset):
    """offset: the destination one float into its allocation, which gives the stereo outputs -- an even number of floats
    apart -- the odd phases as well"""
    import gstpeaq_amd
    import torch
    x = gather_input(channels)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    src = np.array(SRC, np.uint32)
    count = len(SRC) * OUT_STRIDE * channels
    for skip, keep in gather_cases():
        whole = torch.from_numpy(np.full(count + 4, pcm.SENTINEL, np.uint32).view(np.float32)).cuda()
        out = whole[offset:offset + count].view(len(SRC), OUT_STRIDE, channels)
        assert out.data_ptr() == whole.data_ptr() + 4 * offset
        got = gstpeaq_amd.gather(ctx(), d_x, src, skip, keep, out=out)
        torch.cuda.synchronize()
        assert got is out
        bits = whole.cpu().numpy().view(np.uint32)
        assert (bits[:offset] == pcm.SENTINEL).all() and (bits[offset + count:] == pcm.SENTINEL).all()
        bits = bits[offset:offset + count].reshape(len(SRC), OUT_STRIDE, channels)
        for p in range(len(SRC)):
            exp = x[src[p], skip[p]:skip[p] + keep[p]]
            bad = np.argwhere(bits[p, :keep[p]] != exp)
            assert bad.size == 0, (channels, offset, p, int(skip[p]), int(keep[p]), bad[:4])
            assert (bits[p, keep[p]:] == pcm.SENTINEL).all(), (channels, offset, p)          # past n_keep: untouched
    # defaults: no skip, the whole row, a zero-filled destination with an even stride
    full = gstpeaq_amd.gather(ctx(), d_x, src)
    torch.cuda.synchronize()
    assert tuple(full.shape) == (len(SRC), IN_STRIDE + 1, channels)
    full = full.cpu().numpy().view(np.uint32)
    assert (full[:, :IN_STRIDE] == x[src]).all() and not full[:, IN_STRIDE:].any()


@pytest.mark.parametrize("channels", [1, 2])
def test_gather_with_the_identity_equals_cut_bit_for_bit(channels):
    import gstpeaq_amd
    import torch
    x = gather_input(channels)
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    for skip, keep in gather_cases():
        skip, keep = skip[:ROWS], keep[:ROWS]
        outs = [pcm.sentinel_out(ROWS, OUT_STRIDE, channels) for _ in (0, 1)]
        gstpeaq_amd.gather(ctx(), d_x, np.arange(ROWS), skip, keep, out=outs[0])
        gstpeaq_amd.cut(ctx(), d_x, skip, keep, out=outs[1])
        torch.cuda.synchronize()
        a, b = (o.cpu().numpy().view(np.uint32) for o in outs)
        assert (a == b).all(), (channels, skip, keep)
        assert (a[0, :keep[0]] == x[0, skip[0]:skip[0] + keep[0]]).all()


# ---- the feed -----------------------------------------------------------------------------------------------------
REF_INDEX = (0, 1, 0, 2, 0, 2)                       # interleaved: chunks of three split reference 0's tests


@functools.lru_cache(maxsize=None)
def corpus(fmt):
    """three references with 3, 1 and 2 tests and a fourth nobody names, without a buffer.  Reference 0 (48000 samples)
    has a shorter test (47000), a much shorter one (24000) and an empty one; reference 1 (30001) a longer one (33333);
    reference 2 (40960) one of its length and a longer one (44100)."""
    p = pcm.file_pairs(fmt)
    refs = [p[1][0], p[2][0], p[4][0], None]
    tests = [p[1][1], p[2][1], p[0][1], p[4][1], p[3][1], p[8][1]]
    assert [len(t) for t in tests] == [47000, 33333, 24000, 40960, 0, 44100] and [len(r) for r in refs[:3]] == [48000, 30001, 40960]
    return refs, tests


def written_out(refs, tests, ref_index):
    return [(refs[r], t) for r, t in zip(ref_index, tests)]


def refs_rows(refs, tests, ref_index, fmt, advanced, rate=48000, align=None, chunk_pairs=0):
    from gstpeaq_amd import capi
    return capi._run_host_refs_rows(ctx(), advanced, refs, tests, ref_index, fmt, 2, rate, align, chunk_pairs, 92.0)


@functools.lru_cache(maxsize=None)
def expected_rows(fmt, advanced):
    refs, tests = corpus(fmt)
    return pcm.host_rows(written_out(refs, tests, REF_INDEX), fmt, advanced)[0]


@pytest.mark.parametrize("chunk_pairs", [0, 1, 3])
@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
@pytest.mark.parametrize("fmt", ["s16", "s24"])
def test_run_host_refs_equals_run_host_on_the_written_out_pairs(fmt, advanced, chunk_pairs):
    refs, tests = corpus(fmt)
    got, rec = refs_rows(refs, tests, REF_INDEX, fmt, advanced, chunk_pairs=chunk_pairs)
    assert rec is None
    exp = expected_rows(fmt, advanced)
    assert exp[0, 14] >= 40 and exp[5, 14] >= 40        # long enough that the modulation and loudness gates open
    assert_same_rows(got, exp, (fmt, advanced, chunk_pairs))


LATE = (0, 37, -211)


@functools.lru_cache(maxsize=None)
def late_corpus():
    """reference 0 with three tests late by 0, 37 and -211 samples: it is cut differently for each; reference 1 with
    one test of another length"""
    fp = pcm.float_pairs()
    r, t = fp[0]
    refs = [pcm.quantise(r, "s16"), pcm.quantise(fp[2][0], "s16")]
    tests = [pcm.quantise(pcm.shifted(t, LATE[0]), "s16"), pcm.quantise(fp[2][1], "s16"),
             pcm.quantise(pcm.shifted(t, LATE[1]), "s16"), pcm.quantise(pcm.shifted(t, LATE[2]), "s16")]
    return refs, tests, (0, 1, 0, 0)


@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
@pytest.mark.parametrize("rate,align", [(44100, None), (48000, 4096), (44100, 4096)], ids=["44100", "aligned", "44100-aligned"])
def test_run_host_refs_converted_and_aligned_equals_run_host(rate, align, advanced):
    refs, tests, index = late_corpus()
    exp, exp_rec = pcm.host_rows(written_out(refs, tests, index), "s16", advanced, rate=rate, align=align)
    if align and rate == 48000:
        assert [exp_rec[p].lag for p in (0, 2, 3)] == list(LATE)
    for chunk_pairs in (0, 3):
        got, rec = refs_rows(refs, tests, index, "s16", advanced, rate=rate, align=align, chunk_pairs=chunk_pairs)
        assert_same_rows(got, exp, (rate, align, advanced, chunk_pairs))
        if align:
            assert bytes(rec) == bytes(exp_rec), (rate, advanced, chunk_pairs)      # every field of every record
        else:
            assert rec is None
    if align:
        import gstpeaq_amd
        res, delays = gstpeaq_amd.run_host_refs(ctx(), advanced, refs, tests, index, "s16", 2, rate=rate, align=align)
        assert delays["lag"].tolist() == [exp_rec[p].lag for p in range(len(tests))]
        assert np.array([r["odg"] for r in res]).tobytes() == exp[:, 12].tobytes()


def test_a_tests_result_does_not_depend_on_the_other_tests_and_references_of_the_call():
    refs, tests = corpus("s16")
    for advanced in (0, 1):
        exp = expected_rows("s16", advanced)
        alone, _ = refs_rows([refs[0]], [tests[0]], [0], "s16", advanced)
        assert_same_rows(alone, exp[[0]], (advanced, "alone"))
        # the reference list permuted (the unnamed one first), the tests in another order
        perm = [3, 2, 0, 1]                              # new position -> old reference
        where = {old: new for new, old in enumerate(perm)}
        order = [5, 0, 3, 1, 4, 2]
        got, _ = refs_rows([refs[old] for old in perm], [tests[t] for t in order], [where[REF_INDEX[t]] for t in order], "s16",
                           advanced, chunk_pairs=2)
        assert_same_rows(got, exp[order], (advanced, "permuted"))
        # one reference twice in the list, under two indices
        got, _ = refs_rows([refs[0], refs[0]], [tests[0], tests[2]], [1, 0], "s16", advanced)
        assert_same_rows(got, exp[[0, 2]], (advanced, "listed twice"))


# ---- files: run_files(share_refs=) and the CLI's --list ----------------------------------------------------------
@pytest.fixture(scope="module")
def shared_files(tmp_path_factory):
    """six lines: an S16 reference named by four of them, among two S24 pairs with references of their own"""
    d = tmp_path_factory.mktemp("refs")
    fp = pcm.float_pairs()
    ref = d / "ref_shared.wav"
    pcm.write_wav(ref, pcm.quantise(fp[0][0], "s16"), "s16", 48000)
    lines = []
    for k, p in enumerate((0, 1, 2, 4)):
        path = d / f"coded{k}.wav"
        pcm.write_wav(path, pcm.quantise(fp[p][1], "s16"), "s16", 48000)
        lines.append((ref, path))
    for k, p in enumerate((5, 7)):
        paths = (d / f"ref24_{k}.wav", d / f"test24_{k}.wav")
        for path, a in zip(paths, fp[p]):
            pcm.write_wav(path, pcm.quantise(a, "s24"), "s24", 48000)
        lines.insert(1 + 2 * k, paths)
    assert [r == ref for r, _ in lines] == [True, False, True, False, True, True]
    return lines


def test_run_files_shares_references_and_returns_what_it_returned(shared_files):
    import gstpeaq_amd
    shared = gstpeaq_amd.run_files(ctx(), 0, shared_files, share_refs=True)
    plain = gstpeaq_amd.run_files(ctx(), 0, shared_files, share_refs=False)
    assert len(shared) == len(plain) == len(shared_files)
    for i, (a, b) in enumerate(zip(shared, plain)):
        assert pcm.same_result(a, b) and a["frames"] > 20, (i, a, b)
    assert pcm.same_result(gstpeaq_amd.run_files(ctx(), 0, shared_files)[4], plain[4])        # sharing is the default
    (res_a, del_a), (res_b, del_b) = (gstpeaq_amd.run_files(ctx(), 1, shared_files, align=1024, share_refs=s) for s in (True, False))
    assert del_a == del_b and all(pcm.same_result(a, b) for a, b in zip(res_a, res_b))


def test_cli_list_shares_references_and_prints_the_same(shared_files, tmp_path):
    assert pcm.gst_env.CLI.exists(), "gstpeaq_amd/cli/peaq is built by build()"
    path = tmp_path / "pairs.txt"
    path.write_text("# one reference, four codecs\n" + "".join(f"{r}\t{t}\n" for r, t in shared_files))
    shared = pcm.run_cli(f"--list={path}")
    plain = pcm.run_cli(f"--list={path}", "--no-share-refs")
    assert shared.returncode == 0 and plain.returncode == 0, shared.stderr + plain.stderr
    assert shared.stdout == plain.stdout and len(shared.stdout.splitlines()) == len(shared_files)
    assert [line.split("\t")[:2] for line in shared.stdout.splitlines()] == [[str(r), str(t)] for r, t in shared_files]
    assert shared.stderr.splitlines()[-1] == "Note: 3 distinct references read for 6 pairs", shared.stderr
    assert plain.stderr.splitlines()[-1] == "Note: 6 references read for 6 pairs", plain.stderr
