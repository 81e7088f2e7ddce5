"""TimeDomainSpecAugment of the SpeechBrain recipe on the device (ssak_augment_fir_drop in ssak_amd/csrc/augment.hip,
TimeDomainSpecAugmentDevice in ssak_amd/augment.py) against the float64 restatement of its contract (tests/tdsa_ref.py): the FIR
exactly on integers and at the fp32 dot-product bound on real values, chunk zeroing, argument checks, the whole pipeline on a
ragged batch and its independence of the batch split, and the recipe's command line end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tdsa_ref as R  # noqa: E402

from ssak_amd import augment as A  # noqa: E402
from ssak_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = hip.AUG_FIR_TILE  # outputs of one workgroup
HALO = R.TAPS - 1        # samples a tile reads beyond its own


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _chunk_table(rows, max_chunks):
    ch = np.zeros((len(rows), max_chunks, 2), dtype=np.int32)
    n = np.zeros(len(rows), dtype=np.int32)
    for b, row in enumerate(rows):
        n[b] = len(row)
        for j, (s, e) in enumerate(row):
            ch[b, j] = (s, e)
    return ch, n


# T': shorter than the filter, equal to it, one tile, a ragged tail; then the kernel's own edges: a tile less and more than one
# sample, two tiles plus the halo less one, and -- rows start at b * T' floats and the kernel shifts a row's tiles by
# (b * T') mod 4 to keep its 16-byte accesses aligned -- one size of each residue mod 4 around the tile
@pytest.mark.parametrize("T", [37, 101, 2048, 2048 + 37, TILE - 1, TILE + 1, 2 * TILE + HALO - 1, TILE + 2, TILE - 3, 1, 3 * TILE])
def test_fir_is_exact_on_small_integers(T):
    rng = np.random.default_rng(T)
    g = rng.integers(-3, 4, R.TAPS).astype(np.float32)
    x = rng.integers(-8, 9, (3, T)).astype(np.float32)  # |partial sums| <= 101 * 3 * 8 < 2^24: exact in fp32 in any order
    want = R.fir(x, g)
    got = hip.augment_fir_drop(_dev(x), _dev(g)).cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(got.astype(np.float64) != want)
    assert len(bad) == 0, f"T={T}: {len(bad)} wrong, first at {bad[:4].tolist()}"


@pytest.mark.parametrize("ntaps", [1, 3, 51, 253, 255])
def test_fir_other_odd_lengths_are_exact_too(ntaps):
    rng = np.random.default_rng(ntaps)
    T = TILE + 300
    g = rng.integers(-3, 4, ntaps).astype(np.float32)
    x = rng.integers(-8, 9, (2, T)).astype(np.float32)
    got = hip.augment_fir_drop(_dev(x), _dev(g)).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), R.fir(x, g))


def test_fir_on_an_unaligned_view_is_exact():
    """A batch that does not start on a 16-byte boundary takes the kernel's 4-byte path."""
    rng = np.random.default_rng(2)
    T = TILE + 5
    g = rng.integers(-3, 4, R.TAPS).astype(np.float32)
    x = rng.integers(-8, 9, (2, T)).astype(np.float32)
    buf = torch.zeros(2 * T + 1, device=DEV)
    xv = buf[1:].view(2, T)
    xv.copy_(_dev(x))
    assert xv.data_ptr() % 16 != 0 and xv.is_contiguous()
    got = hip.augment_fir_drop(xv, _dev(g)).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), R.fir(x, g))


def test_fir_real_values_within_the_fp32_dot_product_bound():
    rng = np.random.default_rng(1)
    g = R.compose([0.12, 0.37, 0.71]).astype(np.float32)
    x = (rng.standard_normal((2, 5000)) * 0.1).astype(np.float32)
    want, bound = R.fir(x, g), R.fir_bound(x, g)
    got = hip.augment_fir_drop(_dev(x), _dev(g)).cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"max |y - ref| = {err.max():.3e}, max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_identity_is_bit_exact():
    rng = np.random.default_rng(3)
    x = _dev((rng.standard_normal((3, TILE + 77)) * 0.1).astype(np.float32))
    # count == 0 and no chunk: apply hands the batch back untouched
    aug = A.TimeDomainSpecAugmentDevice(drop_freq_count_high=0, drop_chunk_count_high=0, speeds=[100], seed=1)
    lens = np.array([TILE + 77, 100, 2000], dtype=np.int32)
    t = aug.draw(1, range(3), lens)
    assert t.taps is None and not t.counts.any() and t.speed == 100
    y, yl = aug.apply(x, _dev(lens), t)
    assert torch.equal(y, x) and torch.equal(yl.cpu(), torch.from_numpy(lens))
    # the kernel without a filter is a copy, and so is the filter of no notch (the unit impulse)
    assert torch.equal(hip.augment_fir_drop(x), x)
    assert torch.equal(hip.augment_fir_drop(x, _dev(R.compose([]).astype(np.float32))), x)


@pytest.mark.parametrize("filtered", [True, False])
def test_chunks_are_zeroed_and_nothing_else_changes(filtered):
    rng = np.random.default_rng(4)
    T, M = TILE + 952, 5
    x = _dev((rng.standard_normal((4, T)) * 0.1 + 0.5).astype(np.float32))
    g = _dev(R.compose([0.2, 0.6]).astype(np.float32)) if filtered else None
    rows = [[],                                                              # n = 0
            [(0, 100), (T - 200, T)],                                        # starts at 0; ends exactly at T'
            [(T - 50, T + 500), (500, 900), (700, 1200), (-10, 5)],          # clipped past T' and before 0; two overlapping
            [(TILE - 3, TILE + 3), (10, 11), (2999, 2999), (1500, 2600), (40, 48)]]  # max_chunks of them; across a tile; empty
    ch, n = _chunk_table(rows, M)
    plain = hip.augment_fir_drop(x, g)
    got = hip.augment_fir_drop(x, g, _dev(ch), _dev(n), n)
    mask = R.drop_chunks(np.ones((4, T)), rows) == 0
    assert mask[1, 0] and mask[1, T - 1] and mask[2, T - 1] and mask[2, 0] and not mask[0].any() and mask.sum() > 2000
    got, plain = got.cpu().numpy(), plain.cpu().numpy()
    assert (got[mask] == 0.0).all() and not np.signbit(got[mask]).any()
    assert np.array_equal(got[~mask].view(np.int32), plain[~mask].view(np.int32))
    # no table at all: the FIR-only output
    assert np.array_equal(hip.augment_fir_drop(x, g, _dev(ch), _dev(np.zeros(4, np.int32)), np.zeros(4, np.int32)).cpu().numpy().view(np.int32),
                          plain.view(np.int32))


def test_bad_arguments_are_refused_before_any_launch():
    x = torch.ones(2, 300, device=DEV)
    out = torch.full_like(x, 7.0)
    g = torch.ones(101, device=DEV)
    ch, n = _chunk_table([[(0, 10)], [(5, 9)]], 2)
    chd, nd = _dev(ch), _dev(n)
    with pytest.raises(ValueError, match="odd"):  # even ntaps
        hip.augment_fir_drop(x, torch.ones(100, device=DEV), out=out)
    with pytest.raises(ValueError, match="at most 255"):  # ntaps > 255
        hip.augment_fir_drop(x, torch.ones(257, device=DEV), out=out)
    with pytest.raises(ValueError, match="overlap"):  # out == x
        hip.augment_fir_drop(x, g, out=x)
    with pytest.raises(ValueError, match="overlap"):  # out inside x
        hip.check(hip.lib.ssak_augment_fir_drop(hip.ptr(x), 1, 300, hip.ptr(g), 101, None, None, None, 0, C.c_void_p(x.data_ptr() + 400), hip.stream()))
    with pytest.raises(ValueError, match="chunks"):  # negative count
        hip.augment_fir_drop(x, g, chd, nd, np.array([1, -1], dtype=np.int32), out=out)
    with pytest.raises(ValueError, match="chunks"):  # a count above max_chunks
        hip.augment_fir_drop(x, g, chd, nd, np.array([3, 1], dtype=np.int32), out=out)
    with pytest.raises(ValueError):  # taps without a length
        hip.check(hip.lib.ssak_augment_fir_drop(hip.ptr(x), 2, 300, None, 101, None, None, None, 0, hip.ptr(out), hip.stream()))
    with pytest.raises(ValueError):  # chunks without the host's counts
        hip.check(hip.lib.ssak_augment_fir_drop(hip.ptr(x), 2, 300, hip.ptr(g), 101, hip.ptr(chd), hip.ptr(nd), None, 2, hip.ptr(out), hip.stream()))
    with pytest.raises(ValueError):
        hip.check(hip.lib.ssak_augment_fir_drop(hip.ptr(x), 2, 0, hip.ptr(g), 101, None, None, None, 0, hip.ptr(out), hip.stream()))
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (x == 1.0).all()  # nothing was launched


def _resample(aug, x, lens, speed):
    """ssak_resample_sinc as the product calls it: the padded batch with its lengths, sample_rate -> sample_rate * speed // 100."""
    B, T = x.shape
    sr = aug.sample_rate
    o, n, w, taps = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    hip.check(hip.lib.ssak_resample_plan(sr, sr * speed // 100, C.byref(o), C.byref(n), C.byref(w), C.byref(taps)))
    host = torch.empty(n.value * taps.value, dtype=torch.float32)
    hip.check(hip.lib.ssak_resample_table(sr, sr * speed // 100, C.c_void_p(host.data_ptr())))
    T2 = R.ceil_div(T * n.value, o.value)
    y = torch.empty(B, T2, device=DEV)
    hip.check(hip.lib.ssak_resample_sinc(hip.ptr(x), hip.ptr(lens), B, T, sr, sr * speed // 100, hip.ptr(host.to(DEV)), hip.ptr(y), T2, None,
                                         hip.stream()))
    return y


@pytest.mark.parametrize("speed", [95, 100, 105])
def test_pipeline_on_a_ragged_batch_and_its_shards(speed):
    seed, lengths = 21, [16000, 9000, 20001]
    rng = np.random.default_rng(5)
    xs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in lengths]

    def batch(ids):
        w = np.zeros((len(ids), max(lengths[i] for i in ids)), dtype=np.float32)
        for j, i in enumerate(ids):
            w[j, :lengths[i]] = xs[i]
        return _dev(w), _dev(np.array([lengths[i] for i in ids], dtype=np.int32))

    aug = A.TimeDomainSpecAugmentDevice(speeds=[speed], seed=seed)
    # the first step whose draw has a filter and chunks in every row (host arithmetic of the restatement)
    step = next(s for s in range(1, 200) if (lambda d: d["freqs"] and all(d["chunks"]))(R.draw(seed, s, range(3), lengths, speeds=(speed,))))
    ref = R.draw(seed, step, range(3), lengths, speeds=(speed,))
    x, lens = batch([0, 1, 2])
    table = aug.draw(step, range(3), lengths)
    y, ylens = aug.apply(x, lens, table)
    o, n = ref["ratio"]
    assert (o, n) == {95: (20, 19), 100: (1, 1), 105: (20, 21)}[speed]
    assert y.shape == (3, R.ceil_div(20001 * n, o)) and ylens.cpu().tolist() == ref["out_lens"] == [R.ceil_div(L * n, o) for L in lengths]
    # stages 2-3 of the restatement on the resampler's own output (stage 1 is the existing, separately tested kernel)
    mid = (_resample(aug, x, lens, speed) if speed != 100 else x).cpu().numpy()
    g = table.taps
    assert np.abs(g.astype(np.float64) - R.compose(ref["freqs"])).max() <= 1e-7
    want = R.drop_chunks(R.fir(mid, g), ref["chunks"])
    bound = R.fir_bound(mid, g)
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    print(f"speed {speed} step {step}: max err / bound = {(err / bound).max():.3f}, chunks {[len(c) for c in ref['chunks']]}")
    assert (err <= bound).all()
    zeroed = R.drop_chunks(np.ones_like(want), ref["chunks"]) == 0
    assert zeroed.any() and (y.cpu().numpy()[zeroed] == 0).all()
    # two shards of the global batch: every utterance's own samples come out the same, bit for bit (each output sample is a
    # fixed-order sum over the row's own samples, and a row is zero from L' on whatever the batch's padding)
    for ids in ([0, 1], [2]):
        xs_, ls_ = batch(ids)
        ys, yl = aug.apply(xs_, ls_, aug.draw(step, ids, [lengths[i] for i in ids]))
        for j, i in enumerate(ids):
            L2 = ref["out_lens"][i]
            assert int(yl[j]) == L2 and torch.equal(ys[j, :L2], y[i, :L2])


# ------------------------------------------------------------------ the recipe's command line
_HPARAMS = """# written by the test: the recipe's keys with hyperpyyaml tags, small sizes
num_epochs: 6
lr: 1.0
lr_wav2vec: 0.0001
sorting: random
batch_size: 4
test_batch_size: 4
min_duration: 0
max_duration: 15
freeze_wav2vec: True
eval_steps: 4
debug: False
seed: 1234
__set_seed: !apply:torch.manual_seed [!ref <seed>]
train: !PLACEHOLDER
valid: !PLACEHOLDER
output_folder_prefix: ''
base_model: !PLACEHOLDER
dnn_neurons: 64
output_neurons: 30
blank_index: 0
model_opt_class: !name:torch.optim.Adadelta
    lr: !ref <lr>
    rho: 0.95
    eps: 1.e-8
lr_annealing_model: !new:speechbrain.nnet.schedulers.NewBobScheduler
    initial_value: !ref <lr>
    improvement_threshold: 0.0025
    annealing_factor: 0.8
    patient: 0
lr_annealing_wav2vec: !new:speechbrain.nnet.schedulers.NewBobScheduler
    initial_value: !ref <lr_wav2vec>
    improvement_threshold: 0.0025
    annealing_factor: 0.9
    patient: 0
"""
_AUGMENTATION = """sample_rate: 16000
augmentation: !new:speechbrain.lobes.augment.TimeDomainSpecAugment
    sample_rate: !ref <sample_rate>
    speeds: [95, 100, 105]
"""


@pytest.mark.timeout(900)
def test_speechbrain_recipe_cli_augments_training_batches_only(tmp_path):
    """`python -m ssak_amd.train_speechbrain` on a synthetic Kaldi corpus with the finetune yaml's TimeDomainSpecAugment block:
    the run ends well and the validation loss falls; against the same yaml with --augmentation=none the validation before any
    step is the same (validation is not augmented) and the training losses differ (training is); a rerun resumes with nothing
    left to do."""
    import dataclasses
    import subprocess
    from ssak_amd import data as D
    from ssak_amd.checkpoint import save_pretrained
    from ssak_amd.config import Wav2Vec2Config
    from ssak_amd.model import Wav2Vec2ForCTC
    from ssak_amd.synth import VOCAB, synth_text, synth_wave
    from oracle import w2v2_ref as W
    rng = np.random.default_rng(0)
    kd = tmp_path / "kaldi"
    (kd / "audio").mkdir(parents=True)
    with open(kd / "wav.scp", "w") as fw, open(kd / "text", "w") as ft, open(kd / "utt2dur", "w") as fd:
        for i in range(12):
            n = int(rng.integers(16000, 24000))
            D.write_wav(str(kd / "audio" / f"u{i}.wav"), synth_wave(rng, n))
            fw.write(f"utt{i} {kd}/audio/u{i}.wav\n")
            ft.write(f"utt{i} {synth_text(rng, 3, 6)}\n")
            fd.write(f"utt{i} {n / 16000:.3f}\n")
    oc = dataclasses.replace(W.W2V2Config.tiny(), layerdrop=0.0)
    d = dataclasses.asdict(oc)
    d.pop("initializer_range")
    base = Wav2Vec2ForCTC(Wav2Vec2Config(**d))
    base.load_state_dict(W.init_params(oc, 1))
    save_pretrained(base, D.CharTokenizer(VOCAB), str(tmp_path / "base"))
    del base
    hp = tmp_path / "hparams.yaml"
    hp.write_text(_HPARAMS + _AUGMENTATION)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(prefix, *extra):
        cmd = [sys.executable, "-m", "ssak_amd.train_speechbrain", str(hp), f"--train={kd}", f"--valid={kd}", f"--base_model={tmp_path / 'base'}",
               f"--output_folder_prefix={tmp_path}/{prefix}_", "--valid_before_training=true", *extra]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs = [p for p in os.listdir(tmp_path) if p.startswith(prefix + "_sb_")]
        assert len(runs) == 1
        return r, open(tmp_path / runs[0] / "train_log.txt").read().strip().split("\n")

    def column(lines, key):
        return [float(l.split(key)[1].split(",")[0].split(" ")[0]) for l in lines if key in l]

    r, lines = run("aug")
    assert "TimeDomainSpecAugmentDevice" in r.stdout
    assert lines[0].startswith("epoch: 0,") and len(lines) >= 7
    vloss = column(lines, "valid loss: ")
    assert len(vloss) == len(lines) and vloss[-1] < vloss[0] and vloss[-1] < vloss[1]
    r0, clean = run("clean", "--augmentation=none")
    assert "augmentation of training batches" not in r0.stdout
    assert clean[0] == lines[0]  # the validation before any step: validation batches are not augmented
    assert len(clean) == len(lines)
    ta, tc = column(lines, "train loss: "), column(clean, "train loss: ")
    assert len(ta) == len(lines) - 1 and ta != tc and ta[0] != tc[0]
    r2, again = run("aug")
    assert "resuming from" in r2.stdout and again == lines  # nothing left to train
