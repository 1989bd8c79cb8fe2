"""Host-side tests of the resampler: the float64 oracle (tests/resample_reference.py) against scipy's polyphase FIR and
against tones, audio.py's table builder against the oracle, the refusals of audio.resample, and the surfaces that must
not need a GPU (load_wav on a file already at the rate, the --resample flag)."""
import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal
import torch

from fastvocoder_amd import _native, audio
from tests import resample_reference as rr

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000)


@pytest.mark.parametrize("sr_in,sr_out", rr.PAIRS)
def test_oracle_equals_scipy_resample_poly(sr_in, sr_out):
    x = np.random.RandomState(3).uniform(-1, 1, 3000)
    L, M, hf = rr.scipy_fir(sr_in, sr_out)
    want = scipy.signal.resample_poly(x, L, M, window=hf) / L       # resample_poly multiplies a given window by `up`
    got = rr.resample(x, sr_in, sr_out)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"{sr_in} -> {sr_out}: max |oracle - resample_poly| = {err:.2e}")
    assert err <= 1e-10, err


def test_oracle_output_range_equals_the_whole():
    x = np.random.RandomState(4).uniform(-1, 1, 5000)
    full = rr.resample(x, 44100, 24000)
    assert np.array_equal(rr.resample(x, 44100, 24000, 1000, 1700), full[1000:1700])
    assert np.array_equal(rr.resample(x, 44100, 24000, len(full) - 5), full[-5:])


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 24000), (22050, 24000), (48000, 22050)])
def test_output_length(sr_in, sr_out):
    L, M, _, _ = rr.geometry(sr_in, sr_out)
    for n in (1, 2, 147, 320, 1000, 4097):
        want = int(np.ceil(n * L / M))
        assert rr.out_len(n, L, M) == want
        assert len(rr.resample(np.ones(n), sr_in, sr_out)) == want


def test_tone_response_48k_to_24k():
    t = np.arange(6000) / 48000.0
    gains = {}
    for f in (1000, 10000, 12700, 14000):
        x = np.sin(2 * np.pi * f * t)
        y = rr.resample(x, 48000, 24000)
        gains[f] = float(np.sqrt(np.mean(y[400:-400] ** 2)) * np.sqrt(2))      # a unit sine's RMS is 1 / sqrt(2)
    print(gains)
    assert abs(gains[1000] - 1) <= 2e-3 and abs(gains[10000] - 1) <= 2e-3, gains
    assert gains[12700] <= 1e-6 and gains[14000] <= 1e-6, gains


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 24000), (48000, 22050)])
def test_host_table_equals_the_oracle_coefficients(sr_in, sr_out):
    """audio's table is tap-major [taps, L] in fp32; transposed it is the oracle's [L, taps], rounded once."""
    L, M, _, half = rr.geometry(sr_in, sr_out)
    tab = audio._resample_table_host(sr_in, sr_out)
    assert tab.dtype == np.float32 and tab.shape == (2 * half + 2, L) and tab.flags.c_contiguous
    H = rr.coefficients(sr_in, sr_out)
    # two float64 evaluations (np.i0 / scipy.special.i0) a few ulps of float64 apart, then one rounding to fp32
    assert np.all(np.abs(tab.T.astype(np.float64) - H) <= 2.0 ** -24 * np.abs(H) + 1e-14)
    assert audio._resample_geometry(sr_in, sr_out)[:2] == (L, M) and audio._resample_geometry(sr_in, sr_out)[3] == half


def test_every_pair_of_the_usual_rates_is_within_the_cap():
    for a in RATES:
        for b in RATES:
            L, M, _, half = audio._resample_geometry(a, b)
            assert (2 * half + 2) * L <= _native.RESAMPLE_MAX_TABLE_FLOATS


def test_refusals():
    x = np.zeros(100, dtype=np.float32)
    for bad in ((44100.0, 24000), (44100, 24000.5), (0, 24000), (44100, -1), ("44100", 24000), (True, 24000)):
        with pytest.raises(ValueError, match="positive integers"):
            audio.resample(x, *bad)
    with pytest.raises(ValueError, match="22051"):
        audio.resample(x, 44100, 22051)                  # L = 22051: a table of 6 million floats
    with pytest.raises(ValueError):
        audio.resample(x, 1000000, 1000)                 # a window beyond the LDS of a block
    with pytest.raises(ValueError, match="empty"):
        audio.resample(np.zeros(0, dtype=np.float32), 48000, 24000)
    with pytest.raises(ValueError):
        audio.resample(np.zeros((2, 100), dtype=np.float32), 48000, 24000)
    with pytest.raises(_native.NativeError, match="ROCm device"):
        audio.resample(torch.zeros(100), 48000, 24000)   # a CPU tensor: no host path


def test_equal_rates_return_the_input_without_a_launch():
    x = np.random.RandomState(5).uniform(-1, 1, 50)
    got = audio.resample(x, 24000, 24000)
    assert got.dtype == np.float32 and np.array_equal(got, x.astype(np.float32))


def test_load_wav_at_the_rate_is_unchanged_by_resample(tmp_path):
    rs = np.random.RandomState(6)
    mono, stereo = str(tmp_path / "mono.wav"), str(tmp_path / "stereo.wav")
    scipy.io.wavfile.write(mono, 24000, (rs.uniform(-0.5, 0.5, 500) * 32767).astype(np.int16))
    scipy.io.wavfile.write(stereo, 24000, rs.uniform(-0.5, 0.5, (500, 2)).astype(np.float32))
    for path in (mono, stereo):
        for encode in (False, True):
            want = audio.load_wav(path, encode=encode)
            for keep in (False, True):
                got = audio.load_wav(path, encode=encode, resample=True, keep_on_device=keep)
                assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)


def test_resample_flag_parses_and_defaults_to_off():
    from fastvocoder_amd.bin import preprocess
    parser = preprocess.build_parser()
    assert parser.parse_args([]).resample is False
    assert parser.parse_args(["--resample"]).resample is True


def test_abi_argument_checks():
    """fv_resample_out_len, and fv_resample's refusals: each call below fails its argument checks, so nothing is launched
    and the placeholder addresses are never read."""
    import ctypes
    lib = _native.lib()
    assert lib.fv_resample_out_len(3000, 80, 147) == 1633
    assert lib.fv_resample_out_len(14_700_000, 147, 320) == 6_752_813
    assert lib.fv_resample_out_len(10, 0, 1) == _native.ERR_INVALID_ARG
    assert lib.fv_resample_out_len(10, 1, (1 << 20) + 1) == _native.ERR_INVALID_ARG
    p = ctypes.c_void_p(4096)

    def call(**kw):
        a = dict(x=p, fmt=_native.PCM_F32, y=p, tab=p, B=1, n_in=1000, n_out=500, L=1, M=2, half=136, stream=None)
        a.update(kw)
        return lib.fv_resample(*a.values())
    assert call(n_out=501) == _native.ERR_INVALID_ARG and b"n_out" in lib.fv_last_error()
    assert call(fmt=2) == _native.ERR_INVALID_ARG
    assert call(n_in=0, n_out=0) == _native.ERR_INVALID_ARG
    assert call(B=0) == _native.ERR_INVALID_ARG
    assert call(tab=None) == _native.ERR_INVALID_ARG
    assert call(half=0) == _native.ERR_UNSUPPORTED
    assert call(L=22051, M=44100, n_out=501, half=136) == _native.ERR_UNSUPPORTED       # the table: 6 million floats
    assert call(L=1, M=1000, n_in=1000, n_out=1, half=67541) == _native.ERR_UNSUPPORTED   # the window: beyond the LDS
