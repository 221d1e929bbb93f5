"""Stage parity of the FFT front end over whole batches: the records of frontend_pair_kernel<109> (the shipped basic
front end), of the two-wave frontend_kernel<109> and of frontend_kernel<55> (gstpeaq_amd/csrc/peaq_frontend.hip) against
the CPU oracle's records of THAT pair and frame, on the populations of tests/fe_stage_cases.py
(tests/test_fe_stage_cases_host.py holds those to what they are meant to be, their conditioning included):

  A  every signal end inside a flush frame -- 0, 1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 2045, 2046, 2047 samples of
     either signal, odd and even ends above 1024, the two signals ending one and many rows apart, a pair without a frame
  B  the item decoding: grids at every remainder modulo 8, 3 and 7 frames per launch (reciprocals of no power of two),
     a second launch of ONE frame (the frames_per_launch == 1 branch) with frame0 = 3 or 7, 70 / 140 items above the
     prefetch distance with the look-ahead landing in pairs whose signal has ended

Every tensor is a view that starts one float into a buffer full of NaN, with an odd pair stride: mono pair bases that
are only 4-byte aligned under the 8-byte loads, and NaN -- not zeros -- behind every signal's end and behind the batch.
The flush frame's zero padding is what the buffer resource's range check returns (FrameSrc::set); a read the check
does not cut shows as a NaN or a wrong value here.

Through existing entries only: debug_frontend_pairs (launched as the batch path launches), debug_select_frontend,
debug_frontend and batch_bands (the batch path itself, with its own chunking).  Bounds: those of
tests/test_gpu_parity.py::test_frontend_records_match_oracle -- unsmeared excitation and loudness^0.3 rtol 2e-10, noise
in bands rtol 1e-6 (flat, atol 0), bandwidths and both flag words exactly, EHS rtol 1e-7 + 1e-13 with NaN where the
oracle has NaN, hop energies rtol 1e-12 -- and of tests/test_gpu_bands.py for the planes: excitations rtol 1e-9, nmr
rtol 1e-6 + 1e-12.  The module prints its largest relative deviation per kernel, population and field at the end of
every run; DESIGN.md 32 has the table measured on an MI355X.  Needs an MI355X (`-m gpu`).

MEASURED on an MI355X, the largest over all populations and the three kernels: unsmeared excitation 7.7e-15, loudness^0.3
2.3e-15, noise in bands 2.4e-12, EHS 2.7e-12 (the pair (2, 2500)), hop energies 0, planes exc 6.8e-15 and nmr 2.4e-12;
every bandwidth and flag the oracle's, no NaN.  No case moved a kernel."""
import numpy as np
import pytest

import fe_stage_cases as fsc
import oracle_lib as orc

pytestmark = pytest.mark.gpu

NB = 109
RAW_ROOT_REF, RAW_ROOT_TEST, RAW_NOISE, RAW_SCAL, RAW_USED, RAW = 0, 112, 224, 336, 343, 352     # peaq_device.h: kRec*
UNSM_REF, UNSM_TEST, LOUD_REF, LOUD_TEST, NOISE, SCAL, PUB = 0, 112, 224, 336, 448, 560, 576      # ... and kPub*
BW, EHS, FLAGS, ENERGIES, UNUSED = slice(560, 562), 562, slice(563, 565), slice(565, 567), slice(567, 576)
KERNELS = {"pair": 0, "two-wave": 1}                 # debug_select_frontend's argument
SENTINEL = -777.25
WORST = {}          # (kernel, population, field) -> (largest relative deviation, where); printed at the end

_ORACLE, _DEVICE, _RUNS, _NORMS = {}, {}, {}, {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    yield gpu_common
    print("\nfront-end stage parity, largest relative deviation from the oracle per kernel, population and field:")
    for (kernel, pop, field), (e, where) in sorted(WORST.items()):
        print(f"  {kernel:9s} {pop:16s} {field:10s} {e:9.2e}  {where}")


def note_worst(kernel, pop, field, err, where):
    key = (kernel, pop, field)
    if err >= WORST.get(key, (-1., ""))[0]:
        WORST[key] = (float(err), where)


def population(pop):
    """"A", "B<n>" (a batch of the remainder series) or "Bbig" -> ([(seed, n_ref, n_test)], frames per launch)"""
    if pop == "A":
        return fsc.a_specs(), 3
    if pop == "Bbig":
        return fsc.b_big_specs(), fsc.B_BIG_FPL
    return fsc.b_specs(int(pop[1:])), fsc.B_FPL


def counts(specs):
    return [orc.count_frames(a, b) for _, a, b in specs]


def oracle(bands, ch, spec):
    """the oracle's records of one pair, [frames, channels, 576]; computed once, shared, never changed"""
    key = (bands, ch, spec)
    if key not in _ORACLE:
        s, a, b = spec
        r, t = fsc.foreign_pair(s, ch, a, b)
        rec = orc.frontend_records(bands, r, t, orc.count_frames(a, b))
        rec.setflags(write=False)
        _ORACLE[key] = rec
    return _ORACLE[key]


def device(specs, ch, stride=None):
    """the packed tensors of a batch on the device -> dict(ref, test = the [pairs, stride, ch] views, n_ref, n_test,
    stride, flat = the two NaN-filled buffers they live in); made once per batch"""
    import torch
    key = (tuple(specs), ch, stride)
    if key not in _DEVICE:
        fr, ft, n_ref, n_test, stride_ = fsc.packed(specs, ch, stride)
        flat = [torch.from_numpy(f).cuda() for f in (fr, ft)]
        ref, test = (fsc.view(f, len(specs), stride_, ch) for f in flat)
        for v, f in ((ref, flat[0]), (test, flat[1])):
            assert v.is_contiguous() and v.data_ptr() - f.data_ptr() == 4 and v.data_ptr() % 8 == 4
        _DEVICE[key] = dict(ref=ref, test=test, n_ref=n_ref, n_test=n_test, stride=stride_, flat=flat)
    return _DEVICE[key]


def run_pairs(gpu, kernel, specs, ch, fpl, stride=None):
    """debug_frontend_pairs of a batch with the basic front end `kernel` at fpl frames per launch -> the raw records
    [pairs, frames, channels, 352], frames = the longest pair's count; one run per argument set, shared"""
    from gstpeaq_amd import capi
    key = (kernel, tuple(specs), ch, fpl, stride)
    if key not in _RUNS:
        d = device(specs, ch, stride)
        ctx = gpu.ctx()
        before = capi.debug_select_frontend(ctx, KERNELS[kernel])
        try:
            raw = capi.debug_frontend_pairs(ctx, d["ref"], d["test"], d["n_ref"], d["n_test"], fpl, max(max(counts(specs)), 1))
        finally:
            capi.debug_select_frontend(ctx, before)
        raw.setflags(write=False)
        _RUNS[key] = raw
    return _RUNS[key]


def rel_dev(got, want):
    """|got - want| / |want|, 0 where both are equal (0 / 0 and NaN = NaN included), inf where only want is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.abs(want)
    return np.where((got == want) | (np.isnan(got) & np.isnan(want)), 0., d)


def norms(gpu):
    """The two per-band factors between the raw record's tenth root and the public record's vectors (peaq_device.h,
    excitation_from_root: unsm = root^10 inv_norm[b], loud = root^3 inv_norm[b]^0.3), from the library's own
    conversion: one even-length stereo pair through debug_frontend and through debug_frontend_pairs, the quotients
    required to be the same for every frame, channel and signal to 1e-13.  (The pair is none of the populations', in
    plain zero-offset tensors: nothing here comes from the values under test.)"""
    if not _NORMS:
        import torch
        import gstpeaq_amd
        from gstpeaq_amd import capi
        r, t = fsc.foreign_pair(fsc.seeds_from(300, 1)[0], 2, 6144, 6144)
        d_r, d_t = torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda()
        pub = gstpeaq_amd.debug_frontend(gpu.ctx(), NB, d_r, d_t, 6)
        raw = capi.debug_frontend_pairs(gpu.ctx(), d_r[None], d_t[None], [6144], [6144], 6, 6)[0]
        assert pub.shape == (6, 2, PUB) and raw.shape == (6, 2, RAW)
        root = np.stack([raw[:, :, RAW_ROOT_REF:RAW_ROOT_REF + NB], raw[:, :, RAW_ROOT_TEST:RAW_ROOT_TEST + NB]])
        assert (root > 0).all()
        r2 = root * root
        q10 = np.stack([pub[:, :, UNSM_REF:UNSM_REF + NB], pub[:, :, UNSM_TEST:UNSM_TEST + NB]]) / (r2 * r2 * (r2 * r2) * r2)
        q3 = np.stack([pub[:, :, LOUD_REF:LOUD_REF + NB], pub[:, :, LOUD_TEST:LOUD_TEST + NB]]) / (r2 * root)
        for q in (q10, q3):
            flat = q.reshape(-1, NB)
            assert (np.abs(flat / flat[0] - 1.) <= 1e-13).all(), float(np.abs(flat / flat[0] - 1.).max())
        inv, inv03 = np.median(q10.reshape(-1, NB), axis=0), np.median(q3.reshape(-1, NB), axis=0)
        np.testing.assert_allclose(inv03, inv ** 0.3, rtol=1e-13, atol=0)
        assert np.array_equal(pub[:, :, NOISE:NOISE + NB], raw[:, :, RAW_NOISE:RAW_NOISE + NB])
        assert np.array_equal(pub[:, :, SCAL:], raw[:, :, RAW_SCAL:], equal_nan=True)
        _NORMS.update(inv=inv, inv03=inv03)
    return _NORMS["inv"], _NORMS["inv03"]


def to_public(gpu, raw):
    """raw records [..., 352] -> the layout of debug_frontend and of the oracle [..., 576], by excitation_from_root's
    own multiplications"""
    inv, inv03 = norms(gpu)
    pub = np.zeros(raw.shape[:-1] + (PUB,))
    for lo_raw, lo_unsm, lo_loud in ((RAW_ROOT_REF, UNSM_REF, LOUD_REF), (RAW_ROOT_TEST, UNSM_TEST, LOUD_TEST)):
        root = raw[..., lo_raw:lo_raw + NB]
        r1 = root * root
        e2 = r1 * r1
        pub[..., lo_unsm:lo_unsm + NB] = e2 * e2 * r1 * inv
        pub[..., lo_loud:lo_loud + NB] = r1 * root * inv03
    pub[..., NOISE:NOISE + NB] = raw[..., RAW_NOISE:RAW_NOISE + NB]
    pub[..., SCAL:] = raw[..., RAW_SCAL:]
    return pub


def record_failures(kernel, pop, bands, got, want, where):
    """got, want: one pair's records [frames, channels, 576].  Every field at test_frontend_records_match_oracle's
    bounds; the largest deviations go into WORST first; -> a list of what does not hold (empty: all is well)"""
    bad = []
    assert got.shape == want.shape, (where, got.shape, want.shape)

    def held(field, lo, n, rtol, atol=0.):
        g, w = got[:, :, lo:lo + n], want[:, :, lo:lo + n]
        dev = rel_dev(g, w)
        f, c, b = np.unravel_index(int(np.argmax(dev)), dev.shape)
        note_worst(kernel, pop, field, dev[f, c, b], f"{where} frame {f} channel {c} index {b}")
        with np.errstate(invalid="ignore"):
            out = ~((np.abs(g - w) <= atol + rtol * np.abs(w)) | (np.isnan(g) & np.isnan(w)))
        if out.any():
            f, c, b = np.argwhere(out)[0]
            bad.append(f"{where}: {field} frame {f} channel {c} index {b}: {g[f, c, b]!r}, the oracle {w[f, c, b]!r} "
                       f"(relative {dev[f, c, b]:.3e}; {int(out.sum())} values beyond the bound)")

    if not np.array_equal(np.isnan(got), np.isnan(want)):
        bad.append(f"{where}: NaN at {np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist()} (frame, channel, index)")
    for field, lo in (("unsm_ref", UNSM_REF), ("unsm_test", UNSM_TEST), ("loud_ref", LOUD_REF), ("loud_test", LOUD_TEST)):
        if bands == 55 and field.endswith("_test"):  # the advanced version reads neither: the 55-band kernel leaves zeros
            if got[:, :, lo:lo + bands].any():
                bad.append(f"{where}: {field} is not zero")
            continue
        held(field, lo, bands, 2e-10)
    held("noise", NOISE, bands, 1e-6)
    held("ehs", EHS, 1, 1e-7, 1e-13)
    held("energies", ENERGIES.start, 2, 1e-12)
    if bands == NB:
        if not np.array_equal(got[:, :, BW], want[:, :, BW]):
            bad.append(f"{where}: bandwidths {got[:, :, BW].tolist()}, the oracle {want[:, :, BW].tolist()}")
    elif got[:, :, BW].any():
        bad.append(f"{where}: bandwidths are not zero")
    if not np.array_equal(got[:, :, FLAGS], want[:, :, FLAGS]):
        bad.append(f"{where}: flags {got[:, :, FLAGS].tolist()}, the oracle {want[:, :, FLAGS].tolist()}")
    for name, sl in (("padding", slice(lo + bands, lo + 112)) for lo in (UNSM_REF, UNSM_TEST, LOUD_REF, LOUD_TEST, NOISE)):
        if got[:, :, sl].any():
            bad.append(f"{where}: {name} {sl.start}:{sl.stop} is not zero")
    if got[:, :, UNUSED].any():
        bad.append(f"{where}: the unused scalars are not zero")
    return bad


def check_batch(gpu, kernel, pop, ch, label):
    """one batch through debug_frontend_pairs against the oracle: every frame a pair has, every field; padding slots,
    unused scalars, frames behind a pair's count and the records of a pair without a frame are 0"""
    specs, fpl = population(pop)
    raw = run_pairs(gpu, kernel, specs, ch, fpl)
    cnt = counts(specs)
    assert raw.shape == (len(specs), max(cnt), ch, RAW)
    bad = []
    for p, (spec, nf) in enumerate(zip(specs, cnt)):
        where = f"pair {p} {spec[1:]}"
        if raw[p, nf:].any() or np.isnan(raw[p, nf:]).any():
            bad.append(f"{where}: records behind its {nf} frames were written")
        for name, sl in (("padding of root_ref", slice(RAW_ROOT_REF + NB, RAW_ROOT_TEST)), ("padding of root_test", slice(RAW_ROOT_TEST + NB, RAW_NOISE)),
                         ("padding of noise", slice(RAW_NOISE + NB, RAW_SCAL)), ("unused scalars", slice(RAW_USED, RAW))):
            if raw[p, :, :, sl].any() or np.isnan(raw[p, :, :, sl]).any():
                bad.append(f"{where}: {name} is not zero")
        if nf:
            bad += record_failures(kernel, label, NB, to_public(gpu, raw[p, :nf]), oracle(NB, ch, spec), where)
    assert not bad, f"{len(bad)} findings: " + " | ".join(bad[:6])


CH = dict(mono=1, stereo=2)
SERIES = [("mono", n) for n in fsc.B_MONO_SIZES] + [("stereo", n) for n in fsc.B_STEREO_SIZES]


# ---- 1, 2: whole batches against the oracle, both basic kernels ------------------------------------------------------
@pytest.mark.parametrize("channels", ["mono", "stereo"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_every_signal_end_matches_the_oracle(gpu, kernel, channels):
    """A: 39 pairs, 55 frames, 3 frames per launch (117 / 234 items, most of which leave at once)"""
    check_batch(gpu, kernel, "A", CH[channels], f"A {channels}")


@pytest.mark.parametrize("channels,n_pairs", SERIES, ids=[f"{c}-{n}" for c, n in SERIES])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_every_grid_remainder_matches_the_oracle(gpu, kernel, channels, n_pairs):
    """B: 3 .. 10 mono and 3 .. 6 stereo pairs of 4 frames at 3 per launch; pair 1 has 2 frames"""
    check_batch(gpu, kernel, f"B{n_pairs}", CH[channels], f"B series {channels}")


@pytest.mark.parametrize("channels", ["mono", "stereo"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_grid_above_the_prefetch_distance_matches_the_oracle(gpu, kernel, channels):
    """B: 10 pairs of 8 frames at 7 per launch, 70 / 140 items, three shorter pairs under the look-ahead"""
    check_batch(gpu, kernel, "Bbig", CH[channels], f"B big {channels}")


# ---- 3: position and launch independence of the pair kernel, bytes -----------------------------------------------------
@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_records_do_not_depend_on_the_frames_per_launch(gpu, channels):
    specs, fpl = population("A")
    at3 = run_pairs(gpu, "pair", specs, CH[channels], fpl)
    for other in (1, 2):
        assert run_pairs(gpu, "pair", specs, CH[channels], other).tobytes() == at3.tobytes(), other


@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_a_pair_alone_gives_the_bytes_it_has_in_the_batch(gpu, channels):
    """five pairs of A as batches of one, with A's stride and offset"""
    specs, fpl = population("A")
    whole = run_pairs(gpu, "pair", specs, CH[channels], fpl)
    stride = fsc.odd_stride(specs)
    for ab in fsc.A_SINGLES:
        p = fsc.A_LENGTHS.index(ab)
        nf = orc.count_frames(*ab)
        alone = run_pairs(gpu, "pair", [specs[p]], CH[channels], fpl, stride)
        assert alone.shape == (1, nf, CH[channels], RAW) and alone[0, :, :, RAW_ROOT_REF:RAW_ROOT_REF + NB].all()
        assert alone[0].tobytes() == whole[p, :nf].tobytes(), ab


@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_a_pair_has_the_same_bytes_in_a_small_and_a_large_grid(gpu, channels):
    """the 4-frame pair with B's first seed: pair 0 of the smallest and of the largest batch of the remainder series"""
    sizes = fsc.b_sizes(CH[channels])
    small = run_pairs(gpu, "pair", fsc.b_specs(min(sizes)), CH[channels], fsc.B_FPL)
    large = run_pairs(gpu, "pair", fsc.b_specs(max(sizes)), CH[channels], fsc.B_FPL)
    assert small[0, :, :, RAW_ROOT_REF:RAW_ROOT_REF + NB].all() and small[0].tobytes() == large[0].tobytes()


# ---- 4: the batch path itself ------------------------------------------------------------------------------------------
def check_bands(gpu, advanced, pop, ch, label):
    """one batch_bands run of a population on its NaN-filled, odd-stride, offset tensors into a row array one pair and one
    frame larger than needed and full of SENTINEL, against the planes computed from the oracle's records"""
    import torch
    import gstpeaq_amd
    bands, row, names = (55, 56, ["exc_ref", "nmr"]) if advanced else (NB, 110, ["exc_ref", "exc_test", "nmr"])
    kernel = "55-band" if advanced else label[0]
    specs, _ = population(pop)
    d, cnt, tab = device(specs, ch), counts(specs), orc.tables(bands)
    whole = torch.full((len(specs) + 1, max(cnt) + 1, ch, len(names), row), SENTINEL, dtype=torch.float64, device="cuda")
    out = gstpeaq_amd.batch_bands(gpu.ctx(), advanced, d["ref"], d["test"], names, d["n_ref"], d["n_test"],
                                  d_bands=whole[:len(specs)])
    assert np.array_equal(out["counts"], cnt)
    whole = whole.cpu().numpy()
    assert (whole[len(specs)] == SENTINEL).all(), "the spare pair's rows were written"
    bad = []
    for p, (spec, nf) in enumerate(zip(specs, cnt)):
        where = f"pair {p} {spec[1:]}"
        assert (whole[p, nf:] == SENTINEL).all(), f"{where}: rows behind its {nf} frames were written"
        if nf == 0:
            continue
        assert (whole[p, :nf, :, :, bands] == 0.).all(), f"{where}: the rows' pad entry"
        want = fsc.planes_from_records(bands, oracle(bands, ch, spec), tab)
        for name in names:
            got = out[name][p, :nf]
            assert got.shape == want[name].shape == (nf, ch, bands)
            if np.isnan(got).any():
                bad.append(f"{where}: {name} is NaN at (frame, channel, band) {np.argwhere(np.isnan(got))[:4].tolist()}")
                continue
            dev = rel_dev(got, want[name])
            f, c, b = np.unravel_index(int(np.argmax(dev)), dev.shape)
            note_worst(kernel, label[1], "plane " + name, dev[f, c, b], f"{where} frame {f} channel {c} band {b}")
            rtol, atol = (1e-6, 1e-12) if name == "nmr" else (1e-9, 0.)
            beyond = np.abs(got - want[name]) > atol + rtol * np.abs(want[name])
            if beyond.any():
                f, c, b = np.argwhere(beyond)[0]
                bad.append(f"{where}: {name} frame {f} channel {c} band {b}: {got[f, c, b]!r}, from the oracle "
                           f"{want[name][f, c, b]!r} (relative {dev[f, c, b]:.3e}; {int(beyond.sum())} values beyond the bound)")
    assert not bad, f"{len(bad)} findings: " + " | ".join(bad[:6])


@pytest.mark.parametrize("channels", ["mono", "stereo"])
@pytest.mark.parametrize("pop", ["A", "Bbig"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_batch_path_basic_planes_match_the_oracle(gpu, kernel, pop, channels):
    """batch_bands, basic version: exc_ref, exc_test and nmr of every frame of every pair, with either basic kernel"""
    from gstpeaq_amd import capi
    ctx = gpu.ctx()
    before = capi.debug_select_frontend(ctx, KERNELS[kernel])
    try:
        check_bands(gpu, 0, pop, CH[channels], (kernel, f"{'A' if pop == 'A' else 'B big'} {channels}"))
    finally:
        capi.debug_select_frontend(ctx, before)


@pytest.mark.parametrize("channels", ["mono", "stereo"])
@pytest.mark.parametrize("pop", ["A", "Bbig"])
def test_batch_path_advanced_planes_match_the_oracle(gpu, pop, channels):
    """batch_bands, advanced version: exc_ref and nmr, that is frontend_kernel<55> in batches of 39 and 10 pairs (the
    filter-bank path of the same run reads the same NaN-filled tensors)"""
    check_bands(gpu, 1, pop, CH[channels], ("55-band", f"{'A' if pop == 'A' else 'B big'} {channels}"))


# ---- 5: the 55-band kernel, one pair per call ----------------------------------------------------------------------------
@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_55_band_records_match_the_oracle(gpu, channels):
    """debug_frontend(55) on six pairs of A where they lie in A's tensors (NaN behind each signal's end; (2500, 0): a
    test signal of no samples): every field test_frontend_records_match_oracle checks, at its bounds, the zeros where
    the 55-band kernel computes nothing included"""
    import gstpeaq_amd
    ch = CH[channels]
    specs, _ = population("A")
    d = device(specs, ch)
    bad = []
    for ab in fsc.A_SINGLES + ((2500, 0),):
        p = fsc.A_LENGTHS.index(ab)
        nf = orc.count_frames(*ab)
        got = gstpeaq_amd.debug_frontend(gpu.ctx(), 55, d["ref"][p], d["test"][p], nf, n_ref=ab[0], n_test=ab[1])
        bad += record_failures("55-band", f"singles {channels}", 55, got, oracle(55, ch, specs[p]), f"pair {p} {ab}")
    assert not bad, f"{len(bad)} findings: " + " | ".join(bad[:6])
