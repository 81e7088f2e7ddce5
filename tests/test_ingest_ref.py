"""CPU: the float64 restatement tests/ingest_ref.py that tests/test_gpu_ingest_kernels.py holds the ingest kernels to, and the
host side of the ingest (ssak_amd.ingest.wav_info / segment_range / read_pcm_segment).

* The reference resampler (every output a gather and a float64 dot product) agrees with the project's fp32 oracle
  (oracle/resample_ref.py, conv1d) on that oracle's own fp32 table, within the fp32 accumulation error of the oracle.
* Its table, rounded to fp32, is the oracle's and the library's (``ssak_resample_table``, a host function) within one fp32
  rounding per tap, and the plans are equal.
* The yardstick of the GPU bar.  A sequential fp32 fused-multiply-add chain (the kernel's own arithmetic, emulated here with an
  exactly rounded fp32 accumulator) against the float64 reference on the same fp32 table, 4001 input samples in [-1, 1], max
  absolute difference over all outputs (measured; the test recomputes them and asserts max <= RESAMPLE_BAR / 2):

      rate pair         random +-1    sine + noise
      44100 -> 16000    4.54e-07      2.01e-07
      22050 -> 16000    3.75e-07      3.09e-07
      11025 -> 16000    2.88e-07      2.29e-07
       8000 -> 16000    2.45e-07      2.18e-07
      12000 -> 16000    2.66e-07      1.95e-07
      24000 -> 16000    2.95e-07      2.24e-07
      32000 -> 16000    4.43e-07      2.18e-07
      48000 -> 16000    3.66e-07      2.36e-07
      96000 -> 16000    3.61e-07      2.74e-07
      16000 ->  8000    4.43e-07      2.18e-07

* The phase quirk.  torchaudio's float32 ``-j / n`` against the exact phase (``quirk=False``), max distance of the float64
  tables / of the outputs for a random +-1 input: 44100 -> 16000 1.9e-06 / 1.0e-05, 22050 -> 16000 7.4e-06 / 2.5e-05,
  11025 -> 16000 1.4e-05 / 3.6e-05; exactly 0 for the other pairs (n = 1, 2, 4: the division is exact in fp32).  An exact-phase
  table is 10 to 36 GPU bars away where it differs at all: a library built on it fails the table comparison here and the
  end-to-end comparison of tests/test_gpu_ingest_kernels.py.
* Host ingest logic on files written into tmp_path: the header walk (plain and WAVE_FORMAT_EXTENSIBLE headers, an odd-sized
  chunk with its pad byte before ``data``, a data chunk longer than the file, the streaming size 0xFFFFFFFF), the segment
  arithmetic of the reference's loader (ssak/utils/audio.py:84-92), and the refusals.
"""
import math
import os
import struct
import sys
import wave

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ingest_ref as IR  # noqa: E402

ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(ROOT, "ssak_amd", "lib", "libssak_hip.so")

# rate pair -> (o, n, width, taps); the pairs of tests/test_gpu_ingest_kernels.py
RATE_PAIRS = {
    (44100, 16000): (441, 160, 17, 475),
    (22050, 16000): (441, 320, 9, 459),
    (11025, 16000): (441, 640, 7, 455),
    (8000, 16000): (1, 2, 7, 15),
    (12000, 16000): (3, 4, 7, 17),
    (24000, 16000): (3, 2, 10, 23),
    (32000, 16000): (2, 1, 13, 28),
    (48000, 16000): (3, 1, 19, 41),
    (96000, 16000): (6, 1, 37, 80),
    (16000, 8000): (2, 1, 13, 28),
}
PAIR_IDS = [f"{a}-{b}" for a, b in RATE_PAIRS]
RESAMPLE_BAR = 1e-6  # the GPU bar of tests/test_gpu_ingest_kernels.py (absolute, inputs in [-1, 1])
U = 2.0 ** -24
N_IN = 4001


def _inputs(seed):
    """(random +-1, sine + noise clipped to [-1, 1]), fp32 values as float64."""
    rng = np.random.default_rng(seed)
    signs = rng.integers(0, 2, N_IN) * 2.0 - 1.0
    t = np.arange(N_IN)
    tone = np.clip(0.6 * np.sin(0.07 * t) + 0.3 * np.sin(1.3 * t + 0.5) + 0.2 * rng.standard_normal(N_IN), -1.0, 1.0)
    return signs, tone.astype(np.float32).astype(np.float64)


def _oracle_table(a, b):
    from oracle import resample_ref as R
    k, width, o, n = R.sinc_resample_kernel(a, b)
    return k.reshape(n, -1).numpy(), (o, n, width, k.shape[-1])


def _f32_spacing(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("pair", list(RATE_PAIRS), ids=PAIR_IDS)
def test_plan_and_table_are_the_oracles_and_the_librarys(pair):
    """(o, n, width, taps) as listed; resample_taps(quirk=True) rounded to fp32 within one fp32 rounding (the spacing at the
    tap) of oracle.resample_ref.sinc_resample_kernel and of ssak_resample_table."""
    a, b = pair
    assert IR.resample_plan(a, b) == RATE_PAIRS[pair]
    mine = IR.resample_taps(a, b).astype(np.float32)
    tab, plan = _oracle_table(a, b)
    assert plan == RATE_PAIRS[pair] and tab.shape == mine.shape
    assert (np.abs(mine.astype(np.float64) - tab) <= _f32_spacing(tab)).all()
    assert np.mean(mine == tab) > 0.99  # (a one-ulp tie-break is rare)
    if not os.path.exists(LIB_PATH):
        pytest.skip("libssak_hip.so is not built: the comparison with ssak_resample_table needs it")
    import ctypes as C
    import ssak_amd.hip as hip
    o, n, w, taps = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    hip.check(hip.lib.ssak_resample_plan(a, b, C.byref(o), C.byref(n), C.byref(w), C.byref(taps)))
    assert (o.value, n.value, w.value, taps.value) == RATE_PAIRS[pair]
    lib_tab = np.full((n.value, taps.value), np.nan, dtype=np.float32)
    hip.check(hip.lib.ssak_resample_table(a, b, C.c_void_p(lib_tab.ctypes.data)))
    assert (np.abs(mine.astype(np.float64) - lib_tab) <= _f32_spacing(lib_tab)).all()
    assert np.mean(mine == lib_tab) > 0.99


def test_exact_phase_differs_from_the_float32_phase():
    """quirk=False is a different filter: the distance recorded in the module docstring (table and outputs, 11025 -> 16000),
    far above the GPU bar, so a kernel or table built on the exact phase fails the GPU comparison."""
    worst_tab = worst_out = 0.0
    for a, b in RATE_PAIRS:
        hq, he = IR.resample_taps(a, b, True), IR.resample_taps(a, b, False)
        d_tab = np.abs(hq - he).max()
        x = _inputs(7)[0]
        d_out = np.abs(IR.resample(x, a, b, taps_f32=hq) - IR.resample(x, a, b, taps_f32=he)).max()
        print(f"quirk vs exact phase {a} -> {b}: table {d_tab:.3e}, outputs (+-1 input) {d_out:.3e}")
        if RATE_PAIRS[(a, b)][1] in (1, 2, 4):  # -j / n is exact in fp32 for n a power of two
            assert d_tab == 0.0
        worst_tab, worst_out = max(worst_tab, d_tab), max(worst_out, d_out)
    assert worst_out > 5 * RESAMPLE_BAR


@pytest.mark.parametrize("pair", list(RATE_PAIRS), ids=PAIR_IDS)
def test_reference_matches_the_fp32_oracle(pair):
    """ingest_ref.resample on the oracle's fp32 table == oracle.resample_ref.resample (fp32 conv1d) within the oracle's own
    accumulation error: per output, taps fp32 roundings of partial sums no larger than S = sum_k |h x|, in any order, taken as
    independent: 4 sqrt(taps) u S (the worst case is taps u S), plus the rounding of the result."""
    from oracle import resample_ref as R
    a, b = pair
    o, n, width, taps = RATE_PAIRS[pair]
    tab, _ = _oracle_table(a, b)
    for x in _inputs(11):
        want = R.resample(x.astype(np.float32), a, b).astype(np.float64)
        got = IR.resample(x, a, b, taps_f32=tab)
        assert got.shape == want.shape == (math.ceil(n * N_IN / o),)
        s_abs = IR.resample(np.abs(x), a, b, taps_f32=np.abs(tab))
        bar = 4.0 * math.sqrt(taps) * U * s_abs + U * np.abs(got) + 1e-12
        err = np.abs(got - want)
        print(f"{a} -> {b}: max |ref - oracle| {err.max():.3e}, max of the bar {bar.max():.3e}")
        assert (err <= bar).all(), (err.max(), float((err / bar).max()))


@pytest.mark.parametrize("pair", list(RATE_PAIRS), ids=PAIR_IDS)
def test_fp32_fma_chain_stays_within_half_the_gpu_bar(pair):
    """The kernel's arithmetic (fp32 table, sequential fmaf over the taps), emulated with exact roundings, against the float64
    reference on the same table: the figures of the module docstring.  This ties the GPU bar to the reference arithmetic and
    not to the code under test."""
    a, b = pair
    tab = IR.resample_taps(a, b).astype(np.float32)
    worst = []
    for x in _inputs(3):
        ref = IR.resample(x, a, b, taps_f32=tab)
        emu = IR.resample_fp32_fma(x, a, b, tab)
        worst.append(float(np.abs(emu - ref).max()))
        assert np.abs(ref).max() <= 1.9  # (sum_k |h[j, k]| < 1.9 for every pair: the outputs' magnitude for inputs in [-1, 1])
    print(f"fp32 fma chain {a} -> {b}: +-1 {worst[0]:.2e}, sine + noise {worst[1]:.2e}")
    assert max(worst) <= RESAMPLE_BAR / 2


def test_resample_reference_edges():
    """Lengths 0 and 1, equal rates, and a hand-evaluated output."""
    assert IR.resample(np.zeros(0), 44100, 16000).shape == (0,)
    assert np.array_equal(IR.resample(np.arange(5.0), 16000, 16000), np.arange(5.0))
    h = IR.resample_taps(8000, 16000)  # o = 1, n = 2, width = 7, taps = 15
    y = IR.resample(np.array([1.0]), 8000, 16000)
    assert y.shape == (2,) and y[0] == h[0, 7] and y[1] == h[1, 7]  # x[0] sits under tap `width` of both phases
    x = np.array([0.5, -1.0, 0.25])
    y = IR.resample(x, 8000, 16000)
    assert y.shape == (6,)
    assert y[3] == pytest.approx(h[1, 6] * 0.5 + h[1, 7] * -1.0 + h[1, 8] * 0.25, abs=1e-16)  # q = 1, j = 1: x[1 + k - 7]
    # unit DC gain away from the edges
    y = IR.resample(np.ones(2000), 44100, 16000)
    assert np.abs(y[50:-50] - 1.0).max() < 2e-3


def test_pcm_reference():
    raw8 = bytes([0, 255, 128, 64])
    assert IR.pcm_to_mono(raw8, 1, 1).tolist() == [-1.0, 127 / 128, 0.0, -0.5]
    assert IR.pcm_to_mono(raw8, 2, 1).tolist() == [(-1.0 + 127 / 128) / 2, -0.25]
    raw16 = struct.pack("<4h", -32768, 32767, 1, -1)
    assert IR.pcm_to_mono(raw16, 1, 2).tolist() == [-1.0, 32767 / 32768, 1 / 32768, -1 / 32768]
    assert IR.pcm_to_mono(raw16, 4, 2).tolist() == [(-32768 + 32767 + 1 - 1) / 4 / 32768]
    raw32 = struct.pack("<2i", -2 ** 31, 2 ** 31 - 1)
    assert IR.pcm_to_mono(raw32, 1, 4).tolist() == [-1.0, (2 ** 31 - 1) / 2 ** 31]
    with pytest.raises(ValueError):
        IR.pcm_to_mono(b"\0\0\0", 1, 3)


def test_normalize_reference():
    rng = np.random.default_rng(5)
    x = 0.3 + 0.1 * rng.standard_normal(100)
    x[60:] = np.nan
    y, m = IR.normalize(x, 60)
    assert m.tolist() == [1] * 60 + [0] * 40 and (y[60:] == 0).all()
    assert abs(y[:60].mean()) < 1e-14
    v = np.var(x[:60])
    assert np.mean(y[:60] ** 2) == pytest.approx(v / (v + 1e-7), rel=1e-12)
    y, m = IR.normalize(x, 0)
    assert (y == 0).all() and (m == 0).all()
    y, m = IR.normalize(x[:1], 1)
    assert y.tolist() == [0.0] and m.tolist() == [1]
    y, m = IR.normalize(x[:60])
    assert m.all() and abs(y.mean()) < 1e-14


# ------------------------------------------------------------------------------------------------ host ingest logic
PCM_GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def _fmt(tag, nch, sr, bits, extensible_sub=None):
    block = nch * ((bits + 7) // 8)
    body = struct.pack("<HHIIHH", 0xFFFE if extensible_sub is not None else tag, nch, sr, sr * block, block, bits)
    if extensible_sub is not None:
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", extensible_sub) + PCM_GUID_TAIL
    return b"fmt " + struct.pack("<I", len(body)) + body


def _chunk(cid, body, declared=None):
    return cid + struct.pack("<I", len(body) if declared is None else declared) + body + (b"\0" if len(body) & 1 else b"")


def _riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _put(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def _pcm_bytes(rng, frames, nch, sw):
    return rng.integers(0, 256, frames * nch * sw, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("sw", [1, 2, 4])
@pytest.mark.parametrize("nch", [1, 2, 6])
def test_wav_info_reads_what_the_wave_module_wrote(tmp_path, sw, nch):
    from ssak_amd.ingest import read_pcm_segment, wav_info
    rng = np.random.default_rng(sw * 10 + nch)
    frames, sr = 1237, 22050
    pcm = _pcm_bytes(rng, frames, nch, sw)
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as f:
        f.setnchannels(nch)
        f.setsampwidth(sw)
        f.setframerate(sr)
        f.writeframes(pcm)
    info = wav_info(p)
    assert (info.sample_rate, info.channels, info.sample_width, info.frames, info.data_offset) == (sr, nch, sw, frames, 44)
    raw, rsr, rch, rsw, n = read_pcm_segment(p)
    assert (raw, rsr, rch, rsw, n) == (pcm, sr, nch, sw, frames)
    fb = nch * sw
    raw, _, _, _, n = read_pcm_segment(p, 0.01, 0.03)  # int(220.5) = 220 frames in, int(440.99..) = 440 long: truncated
    assert n == int((0.03 - 0.01) * sr) == 440 and raw == pcm[220 * fb:660 * fb]
    raw, _, _, _, n = read_pcm_segment(p, None, 0.02)
    assert n == 441 and raw == pcm[:441 * fb]
    raw, _, _, _, n = read_pcm_segment(p, 0.05, 9.0)  # `end` past the end of the file
    assert n == frames - 1102 and raw == pcm[1102 * fb:]
    assert read_pcm_segment(p, 0.06, None)[4] == 0  # `start` past it


def test_wav_info_extensible_header_and_odd_chunk(tmp_path):
    """WAVE_FORMAT_EXTENSIBLE (tag 0xFFFE, PCM sub-format) and a LIST chunk of odd size, whose pad byte is not in its size."""
    from ssak_amd.ingest import read_pcm_segment, wav_info
    rng = np.random.default_rng(1)
    pcm = _pcm_bytes(rng, 500, 2, 2)
    p = _put(tmp_path / "ext.wav", _riff(_fmt(1, 2, 16000, 16, extensible_sub=1), _chunk(b"LIST", b"INFOx"), _chunk(b"data", pcm)))
    info = wav_info(p)
    assert (info.sample_rate, info.channels, info.sample_width, info.frames) == (16000, 2, 2, 500)
    assert info.data_offset == 12 + (8 + 40) + (8 + 5 + 1) + 8
    assert read_pcm_segment(p)[0] == pcm
    # the same with the odd chunk between an ordinary fmt chunk and data, and an even one after it
    p = _put(tmp_path / "odd.wav", _riff(_fmt(1, 1, 8000, 8), _chunk(b"LIST", b"abc"), _chunk(b"fact", b"1234"), _chunk(b"data", pcm)))
    info = wav_info(p)
    assert (info.sample_rate, info.channels, info.sample_width, info.frames) == (8000, 1, 1, 2000)
    assert read_pcm_segment(p)[0] == pcm
    # an odd chunk longer than the 4 KiB block the header walk reads first: the data header comes from a read of its own
    p = _put(tmp_path / "big.wav", _riff(_fmt(1, 2, 44100, 16), _chunk(b"LIST", bytes(5001)), _chunk(b"data", pcm)))
    info = wav_info(p)
    assert (info.frames, info.data_offset) == (500, 12 + 24 + (8 + 5001 + 1) + 8)
    assert read_pcm_segment(p, 0.001, None)[0] == pcm[44 * 4:]
    # an EXTENSIBLE header whose sub-format is IEEE float is refused like a plain float header
    p = _put(tmp_path / "extf.wav", _riff(_fmt(1, 1, 16000, 32, extensible_sub=3), _chunk(b"data", pcm)))
    with pytest.raises(RuntimeError, match="extf.wav"):
        wav_info(p)


@pytest.mark.parametrize("declared", [1000 * 4 + 4000, 0xFFFFFFFF])
def test_wav_info_truncated_data_chunk(tmp_path, declared):
    """A data chunk that declares more than the file holds (a cut-off copy; 0xFFFFFFFF from a streaming writer): the frames
    that are there, whole frames only."""
    from ssak_amd.ingest import read_pcm_segment, segment_range, wav_info
    rng = np.random.default_rng(2)
    pcm = _pcm_bytes(rng, 1000, 2, 2) + b"\x7f\x7f\x7f"  # (three bytes of a 1001st frame)
    p = _put(tmp_path / "cut.wav", _riff(_fmt(1, 2, 16000, 16)) + b"data" + struct.pack("<I", declared) + pcm)
    info = wav_info(p)
    assert info.frames == 1000
    assert segment_range(info, None, None) == (info.data_offset, 1000)
    assert read_pcm_segment(p)[0] == pcm[:4000]
    assert segment_range(info, 0.05, 10.0) == (info.data_offset + 800 * 4, 200)


def test_segment_range_follows_the_reference_loader():
    """audio.py:84-92: must_cut = start or end; offset = int(start * sr); nframes = int((end - start) * sr) if end; the reader
    stops at the end of the file."""
    from ssak_amd.ingest import WavInfo, segment_range
    sr, n, nch, sw, off = 22050, 50000, 2, 2, 44
    info = WavInfo(sr, nch, sw, off, n)
    fb = nch * sw

    def ref(start, end):
        if not (start or end):
            return 0, n
        s = float(start if start else 0)
        s0 = min(int(s * sr), n)
        cnt = int((float(end) - s) * sr) if end else n - s0
        return s0, max(0, min(cnt, n - s0))

    cases = [(None, None), (0.0, None), (None, 0.0), (0.0, 0.0), (0.5, None), (None, 1.25), (0.0, 1.25), (0.25, 1.1),
             (0.1, 0.30000000000000004), (1.0, 2.0000001), (2.0, 5.0), (None, 5.0), (2.2675, None), (2.3, None), (3.0, 4.0),
             (1.0, 1.0), ("0.5", "0.75"), (1.5, 1.0)]
    for start, end in cases:
        s0, cnt = ref(start, end)
        assert segment_range(info, start, end) == (off + s0 * fb, cnt), (start, end)
    # spelled out: `end` past the end of the file is clipped, `start` past it leaves nothing, truncation not rounding
    assert segment_range(info, 2.0, 5.0) == (off + 44100 * fb, 5900)
    assert segment_range(info, None, 5.0) == (off, 50000)
    assert segment_range(info, 3.0, 4.0) == (off + 50000 * fb, 0)
    assert segment_range(info, 0.1, 0.30000000000000004) == (off + 2205 * fb, 4410)
    assert segment_range(info, 0.00001, None) == (off, 50000)  # int(0.22) = 0
    # Deliberate divergence, pinned: a segment shorter than one sample, int((end - start) * sr) == 0, is 0 frames here.  The
    # reference hands that 0 to its reader as nframes (audio.py:88-92), where 0 means "to the end of the file"; a training
    # segment of no length must not turn into the rest of the recording, so the product keeps 0.
    assert segment_range(info, 1.0, 1.00001) == (off + 22050 * fb, 0)
    assert segment_range(info, 1.0, 1.0) == (off + 22050 * fb, 0)


def test_wav_info_refusals_name_the_path(tmp_path):
    from ssak_amd.ingest import read_pcm_segment, wav_info
    rng = np.random.default_rng(3)
    pcm = _pcm_bytes(rng, 100, 1, 4)
    bad = {
        "pcm24.wav": _riff(_fmt(1, 1, 16000, 24), _chunk(b"data", pcm[:300])),
        "float.wav": _riff(_fmt(3, 1, 16000, 32), _chunk(b"data", pcm)),
        "order.wav": _riff(_chunk(b"data", pcm), _fmt(1, 1, 16000, 32)),
        "notriff.wav": b"OggS" + pcm,
        "short.wav": b"RIFF\x04\0\0\0",
        "nodata.wav": _riff(_fmt(1, 1, 16000, 16), _chunk(b"LIST", b"abcd")),
        "rifx.wav": b"RIFX" + _riff(_fmt(1, 1, 16000, 16), _chunk(b"data", pcm))[4:],
    }
    for name, data in bad.items():
        p = _put(tmp_path / name, data)
        with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
            wav_info(p)
        with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
            read_pcm_segment(p)
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(RuntimeError, match=r"File not found: .*missing\.wav"):
        wav_info(missing)
    os.mkdir(str(tmp_path / "dir.wav"))
    with pytest.raises(RuntimeError, match=r"dir\.wav"):
        wav_info(str(tmp_path / "dir.wav"))
    # (a 24-bit file written by the wave module, header as a real one has it)
    p = str(tmp_path / "w24.wav")
    with wave.open(p, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(3)
        f.setframerate(16000)
        f.writeframes(pcm[:300])
    with pytest.raises(RuntimeError, match=r"w24\.wav"):
        wav_info(p)
