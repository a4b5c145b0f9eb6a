"""CPU: step 1 (hypotremormcmc_amd.convert) -- the numpy restatement against a literal transcription of the reference's
loops, the constants, the SAC reader, file names, time IDs and the parameter keys; the exact FFT references and bounds
of tests/fft_restatement.py against np.fft.  The GPU side is in test_gpu_convert.py and test_gpu_fft.py."""
import ctypes as C
import math

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, convert, synth
from hypotremormcmc_amd.param import REQUIRED_CONVERT, Param
from tests import convert_restatement as cr
from tests import fft_restatement as fr


@pytest.mark.parametrize("n", [12, 20, 40])
@pytest.mark.parametrize("h", [0, 1, 3])
def test_restatement_equals_literal_loop(n, h):
    n2 = n // 2
    rng = np.random.default_rng(n * 10 + h)
    for N in sorted({n, n + 1, n + n2 - 1, n + n2, n + 3 * n2, n + 3 * n2 + 1, n + 2 * n2 + n2 - 1}):
        for n_fac in (1, 3, n // 4):
            if 2 * h > n or n_fac > n2:
                continue
            x1, x2 = rng.standard_normal(N), rng.standard_normal(N) * 3 + 5.0
            kb = (1, 2, n // 3, n // 2 - 1)
            lit = cr.convert_literal(x1, x2, n, n_fac, h, kb, (1.3, 0.7))
            vec = cr.convert(x1, x2, n, n_fac, h, kb, (1.3, 0.7))
            assert vec.size == lit.size == math.ceil(N / n_fac), (N, n_fac)
            np.testing.assert_allclose(vec, lit, rtol=1e-12, atol=1e-12 * np.max(np.abs(lit)))
            k0, cnt = convert.outputs(N, n, n_fac, 0, convert.last_segment(N, n))
            assert (k0, cnt) == (0, lit.size)


def test_smoothing_windows():
    rng = np.random.default_rng(1)
    for n, h in ((12, 0), (12, 1), (12, 3), (40, 3), (40, 20)):
        x = rng.standard_normal(n)
        np.testing.assert_allclose(cr.smooth(x, h), cr.smooth_loop(x, h), rtol=0, atol=1e-13)
    assert np.all(cr.smooth(np.ones(12), 0) == 0.0)


def test_segments_tile_the_record():
    for n in (12, 40, 3000):
        for N in (n, n + 1, n + n // 2 - 1, n + n // 2, n + 7 * n // 2 + 5):
            segs = cr.segments(N, n)
            assert segs[0][1] == 0 and segs[-1][2] == N
            assert all(a[2] == b[1] for a, b in zip(segs, segs[1:]))
            assert convert.last_segment(N, n) == len(segs) - 1
            for j, s, e in segs:
                assert convert.kept_range(j, N, n) == (s, e)
            for n_fac in (1, 7, n // 4):
                ks = [convert.outputs(N, n, n_fac, j, j) for j, _, _ in segs]
                assert ks[0][0] == 0 and sum(c for _, c in ks) == -(-N // n_fac)
                assert all(a[0] + a[1] == b[0] for a, b in zip(ks, ks[1:]))


def test_short_record_and_bad_n_refused():
    x = np.zeros(11)
    with pytest.raises(ValueError, match="not enough"):
        cr.convert(x, x, 12, 1, 1, (1, 2, 3, 4))
    with pytest.raises(ValueError, match="not enough"):
        cr.convert_literal(x, x, 12, 1, 1, (1, 2, 3, 4))
    with pytest.raises(ValueError, match="multiple of 4"):
        cr.convert(np.zeros(30), np.zeros(30), 14, 1, 1, (1, 2, 3, 4))
    c = convert.constants(1.0, 12.0)
    with pytest.raises(SystemExit, match="not enough"):
        convert.check_constants(c, 11)
    with pytest.raises(SystemExit, match="n4"):
        convert.check_constants(convert.constants(1.0, 14.0), 100)
    with pytest.raises(SystemExit, match="n2"):
        convert.check_constants(convert.constants(1.0, 13.0), 100)


def test_constants_from_float32_delta():
    c = convert.constants(float(np.float32(0.05)), 3000.0)
    assert (c.n, c.n_fac, c.h) == (60000, 20, 29)
    assert c.k_band[3] == c.n // 2                  # f4 = 10 Hz is the Nyquist frequency at 20 Hz
    c = convert.constants(float(np.float32(0.01)), 3000.0)
    assert (c.n, c.n_fac, c.h) == (300000, 100, 150)
    assert c.k_band == (3000, 9000, 24000, 30000)
    c = convert.constants(float(np.float32(0.1)), 3000.0)      # 10 Hz: f3, f4 above Nyquist
    assert c.k_band[2] > c.n // 2 and c.n_fac == 10


@pytest.mark.parametrize("delta,t_win", [(0.01, 3000.0), (0.05, 3000.0), (0.01, 30.0)])
def test_closed_form_in_restatement(delta, t_win):
    c = convert.constants(float(np.float32(delta)), t_win)
    n, n2, n4 = c.n, c.n // 2, c.n // 4
    cyc = (c.k_band[1] + c.k_band[2]) // 2
    assert c.k_band[1] <= cyc < c.k_band[2] and cyc < n2
    N = n + 2 * n2
    m = np.arange(N)
    A = 3.5
    x = A * np.cos(2 * math.pi * cyc * m / n)
    want = cr.closed_form(A, c.h)
    for j in range(3):
        seg = x[j * n2:j * n2 + n]
        e = cr.process_segment(seg, np.zeros(n), c.h, c.k_band, (1.0, 1.0))
        err = np.max(np.abs(e[n4:n - n4] - want)) / want
        assert err < 1e-9, err


def test_sac_reader_both_byte_orders(tmp_path):
    x = np.arange(1000, dtype=np.float32) * 0.25 - 7
    for big in (False, True):
        p = str(tmp_path / f"a{int(big)}.sac")
        synth.write_sac(p, x, 0.01, big_endian=big)
        f = convert.read_sac_header(p)
        assert f.order == (">" if big else "<") and f.npts == 1000
        assert f.delta == float(np.float32(0.01))
        assert np.array_equal(f.read(), x)
        assert np.array_equal(f.read(10, 20), x[10:20])
    p7 = str(tmp_path / "v7.sac")
    synth.write_sac(p7, x, 0.01, nvhdr=7)
    assert convert.read_sac_header(p7).npts == 1000


def test_sac_reader_refusals(tmp_path):
    x = np.ones(100, dtype=np.float32)
    bad = str(tmp_path / "bad.sac")
    synth.write_sac(bad, x, 0.01, nvhdr=5)
    with pytest.raises(SystemExit, match="bad.sac"):
        convert.read_sac_header(bad)
    short = str(tmp_path / "short.sac")
    synth.write_sac(short, x, 0.01)
    with open(short, "r+b") as f:
        f.truncate(632 + 4 * 99)
    with pytest.raises(SystemExit, match="short.sac"):
        convert.read_sac_header(short)
    with pytest.raises(SystemExit, match="missing.sac"):
        convert.read_sac_header(str(tmp_path / "missing.sac"))


def _two_ids(tmp_path, d2=0.01, npts2=(500, 500)):
    paths = []
    for k, (d, npts) in enumerate(((0.01, (500, 500)), (d2, npts2))):
        pair = []
        for c in range(2):
            p = str(tmp_path / f"id{k}.c{c}")
            synth.write_sac(p, np.ones(npts[c], dtype=np.float32), d)
            pair.append(p)
        paths.append(tuple(pair))
    return paths


def test_delta_and_npts_checks(tmp_path):
    st = convert.plan_station("S", _two_ids(tmp_path), (1.0, 1.0), 4.0)
    assert st.n_total == 1000 and st.c.n == 400
    (tmp_path / "a").mkdir()
    with pytest.raises(SystemExit, match="delta.*id1.c0"):
        convert.plan_station("S", _two_ids(tmp_path / "a", d2=0.010002), (1.0, 1.0), 4.0)
    (tmp_path / "b").mkdir()
    st = convert.plan_station("S", _two_ids(tmp_path / "b", d2=0.0100005), (1.0, 1.0), 4.0)     # within 1.e-6
    assert st.n_total == 1000
    (tmp_path / "c").mkdir()
    with pytest.raises(SystemExit, match="npts.*id1.c0.*id1.c1"):
        convert.plan_station("S", _two_ids(tmp_path / "c", npts2=(500, 499)), (1.0, 1.0), 4.0)


def test_station_reads_across_files(tmp_path):
    x = [np.arange(k * 1000, k * 1000 + 300 + 7 * k, dtype=np.float32) for k in range(3)]
    paths = []
    for k in range(3):
        pair = []
        for c in range(2):
            p = str(tmp_path / f"f{k}{c}")
            synth.write_sac(p, x[k] * (1 + c), 0.01, big_endian=(k == 1))
            pair.append(p)
        paths.append(tuple(pair))
    st = convert.plan_station("S", paths, (1.0, 1.0), 4.0)
    allx = np.concatenate(x)
    a, b = st.read(250, 620)
    assert np.array_equal(a, allx[250:620]) and np.array_equal(b, 2 * allx[250:620])


def test_filenames_and_time_ids(tmp_path):
    assert convert.expand_filename("data", "$STA+/+$ID+.+$CMP", "ST1", "20200101", "EH1") == "data/ST1/20200101.EH1"
    assert convert.expand_filename("d", "raw_+$ID+_+$STA+.sac.+$CMP", "A", "x", "Z") == "d/raw_x_A.sac.Z"
    p = tmp_path / "ids"
    p.write_text("2020.001  \n 2020.002\n\n2020.003")
    assert convert.read_time_ids(str(p)) == ["2020.001", " 2020.002", "", "2020.003"]


def test_required_keys_and_message(tmp_path):
    assert REQUIRED_CONVERT == ["n_procs", "station_file", "data_dir", "time_id_file", "cmp1", "cmp2",
                                "filename_format", "t_win_conv"]
    (tmp_path / "st").write_text("A 0 0 0 1 1\n")
    keys = dict(n_procs=1, station_file=str(tmp_path / "st"), data_dir="d", time_id_file="t", cmp1="a", cmp2="b",
                filename_format="$ID", t_win_conv=100.0)
    for drop in REQUIRED_CONVERT:
        p = tmp_path / f"p_{drop}"
        p.write_text("".join(f"{k} = {v}\n" for k, v in keys.items() if k != drop))
        with pytest.raises(SystemExit, match=f"ERROR: {drop} is not given."):
            Param(str(p), from_where="convert")
    p = tmp_path / "p_all"
    p.write_text("".join(f"{k} = {v}\n" for k, v in keys.items()))
    para = Param(str(p), from_where="convert")
    assert para.values["filename_format"] == "$ID" and para.values["t_win_conv"] == 100.0
    assert np.array_equal(para.sta_amp_fac, [[1.0, 1.0]])


def test_new_entry_points_refuse_without_device():
    lib = _lib.load()
    n = C.c_int(-1)
    rc = lib.htm_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present; the no-device behaviour is exercised on the CPU-only container")
    x = np.zeros(2 * 8)
    dp = x.ctypes.data_as(_lib.dp)
    assert lib.htm_fft(0, dp, 8, dp, 8, 8, 1, -1) == -2
    assert lib.htm_fft_dev(0, C.c_void_p(1), 8, C.c_void_p(2), 8, 8, 1, -1, None) == -2
    f = np.zeros(64, dtype=np.float32)
    fp = f.ctypes.data_as(C.POINTER(C.c_float))
    kb = (C.c_int * 4)(1, 2, 3, 4)
    out = np.zeros(64)
    assert lib.htm_convert(0, fp, fp, 64, 16, 1, 1, kb, 1.0, 1.0, 0, 0, out.ctypes.data_as(_lib.dp)) == -2
    assert lib.htm_convert_dev(0, C.c_void_p(1), C.c_void_p(1), 64, 16, 1, 1, kb, 1.0, 1.0, 0, 0, C.c_void_p(1),
                               None) == -2
    # bad shapes are refused before any device call
    assert lib.htm_convert(0, fp, fp, 64, 18, 1, 1, kb, 1.0, 1.0, 0, 0, out.ctypes.data_as(_lib.dp)) == -1
    assert lib.htm_convert(0, fp, fp, 15, 16, 1, 1, kb, 1.0, 1.0, 0, 0, out.ctypes.data_as(_lib.dp)) == -1
    assert lib.htm_fft(0, dp, 8, dp, 8, (1 << 24) + 1, 1, -1) == -1
    assert lib.htm_fft(0, dp, 8, dp, 8, 8, 1 << 30, -1) == -1
    assert lib.htm_fft(0, dp, 8, dp, 8, 8, 1, 0) == -1


def test_batches_budget():
    assert convert.batch_segments(300000, 512) >= 10
    assert convert.batch_segments(300000, 1) == 1
    assert convert.batch_segments(4 * 75011, 512) >= 1


@pytest.mark.parametrize("n", [1, 2, 3, 7, 12, 105, 343, 1024, 3000])
def test_numpy_fft_within_stockham_bound_of_exact_dft(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    for d, got in ((-1, np.fft.fft(x, axis=1)), (1, np.fft.ifft(x, axis=1) * n)):
        ref = fr.dft_exact(x, d)
        assert ref.dtype == np.clongdouble
        err = np.linalg.norm((got - ref).astype(np.complex128), axis=1) / np.linalg.norm(ref.astype(np.complex128), axis=1)
        assert np.all(err <= fr.stockham_bound(n)), (n, d, err, fr.stockham_bound(n))


def test_fft_restatement_pass_lists_and_bounds():
    assert fr.passes(300000) == [4, 4, 2, 3, 5, 5, 5, 5, 5]
    assert fr.passes(1) == [] and fr.passes(2) == [2] and fr.passes(1024) == [4] * 5 and fr.passes(2048) == [4] * 5 + [2]
    assert fr.passes(105) == [3, 5, 7] and fr.passes(28) == [4, 7]
    assert fr.passes(11) is None and fr.passes(4 * 75011) is None
    assert (fr.inner_length(11), fr.inner_length(33), fr.inner_length(1009), fr.inner_length(2018)) == (32, 128, 2048, 4096)
    u = 2.0 ** -53
    assert fr.stockham_bound(1) == 0.0 and fr.stockham_bound(2048) == 29 * u
    assert abs(fr.stockham_bound(28) / u - (8 + 9 * math.sqrt(7))) < 1e-12
    assert abs(fr.stockham_bound(300000) / u - (5 + 5 + 4 + 3 + 5 * math.sqrt(3) + 5 * (3 + 7 * math.sqrt(5)))) < 1e-12
    for n in (11, 33, 129, 1009):
        assert 2.0 < fr.kappa(n) < 2.3
        three = fr.kappa(n) * (3 * fr.stockham_bound(fr.inner_length(n)) + 7 * u) + 3 * u      # three equal transforms
        assert abs(fr.bluestein_bound(n) / three - 1) < 1e-12
        assert fr.bluestein_bound(n, 4.0) < 1e-12


def test_fft_restatement_impulse_and_tone_are_the_exact_dft():
    for n in (1, 2, 7, 12, 33):
        for d in (-1, 1):
            for j in sorted({0, 1 % n, n - 1}):
                e = np.zeros(n)
                e[j] = 1.0
                assert np.max(np.abs(fr.dft_exact(e, d) - fr.impulse_spectrum(n, j, d))) == 0
                line = fr.dft_exact(fr.tone(n, j, d), d)
                want = np.zeros(n)
                want[j] = n
                assert np.max(np.abs(line - want)) < 1e-17 * n * n
    c, s = fr.roots(16)
    assert c[4] == 0 and s[4] == 1 and c[8] == -1 and s[8] == 0 and c[2] == s[2] and c[14] == -s[14]
    assert fr.impulse_spectrum(24, 5, -1, 3, 7).shape == (4,)
