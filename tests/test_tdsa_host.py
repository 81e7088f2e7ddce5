"""CPU: the SpeechBrain recipe's TimeDomainSpecAugment on the host side (ssak_amd/augment.py, ssak_amd/train_speechbrain.py)
against the float64 restatement of its contract (tests/tdsa_ref.py): the notch filter's properties and orientation, the
product's taps, the draws and their independence of the batch split, and the yaml dispatch."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tdsa_ref as R  # noqa: E402

FINETUNE_BLOCK = """
sample_rate: 16000
augmentation: !new:speechbrain.lobes.augment.TimeDomainSpecAugment
    sample_rate: !ref <sample_rate>
    speeds: [95, 100, 105]
"""
SPEECH_AUGMENT_BLOCK = """
sample_rate: 16000
augmentation: !new:ssak.utils.augment.SpeechAugment
    sample_rate: !ref <sample_rate>
    noise_dir: /corpus/noise
    rir_dir: /corpus/rirs
    rir_lists: [small/rir_list, large/rir_list]
    apply_prob: 1
    verbose: False
"""


# ------------------------------------------------------------------ the notch
@pytest.mark.parametrize("f", [0.1, 0.3, 0.5, 0.8])
def test_notch_sums_to_one_and_rejects_its_band(f):
    h = R.notch(f)
    assert abs(h.sum() - 1.0) < 1e-12
    H = np.abs(np.fft.rfft(h, 8192))
    grid = np.arange(len(H)) / (len(H) - 1)  # in units of Nyquist
    k = int(np.argmin(H))
    assert H[k] < 0.02
    assert abs(grid[k] - 3 * (f + 0.05) / np.pi) < 0.02
    assert H.max() < 1.01


def test_orientation_is_cross_correlation():
    freqs = [0.12, 0.37, 0.71]
    g = R.compose(freqs)
    g_conv = R.compose(freqs, op=R.convolve_same)
    assert np.abs(g - g_conv).max() > 1e-3
    # the restatement's correlation is numpy's
    h = R.notch(0.3)
    assert np.allclose(R.correlate_same(h, h), np.correlate(np.pad(h, 50), h, mode="valid"), rtol=0, atol=1e-15)


@pytest.mark.parametrize("freqs", [[0.4], [0.12, 0.37], [0.12, 0.37, 0.71], [1e-14, 0.999]])
def test_product_taps_match_the_reference(freqs):
    from ssak_amd import augment as A
    for f in freqs:
        assert np.abs(A.notch_filter(f) - R.notch(f)).max() < 1e-14
    got = A.compose_notches(freqs).astype(np.float32)
    want = R.compose(freqs)
    assert got.shape == (101,) and np.abs(got.astype(np.float64) - want).max() <= 1e-7


# ------------------------------------------------------------------ draws
def _same_rows(t, ref, rows):
    for b in rows:
        n = int(t.counts[b])
        assert [tuple(int(v) for v in c) for c in t.chunks[b, :n]] == ref["chunks"][b]


def _check(t, ref):
    assert t.speed == ref["speed"] and tuple(t.ratio) == ref["ratio"]
    assert [float(f) for f in t.freqs] == ref["freqs"]
    assert [int(v) for v in t.out_lens] == ref["out_lens"]
    _same_rows(t, ref, range(len(ref["chunks"])))
    if ref["freqs"]:
        assert np.abs(t.taps.astype(np.float64) - R.compose(ref["freqs"])).max() <= 1e-7 and t.taps.dtype == np.float32
    else:
        assert t.taps is None


def test_draws_follow_the_contract_and_do_not_depend_on_the_split():
    from ssak_amd.augment import TimeDomainSpecAugmentDevice
    aug = TimeDomainSpecAugmentDevice(seed=7)
    lengths = [16000, 9000, 20001, 31000, 1500, 800, 48000, 16001]
    seen = set()
    for step in range(1, 13):
        whole = aug.draw(step, range(8), lengths)
        _check(whole, R.draw(7, step, range(8), lengths))
        # two ranks' shards of the same global batch, drawn separately
        for pos in (range(0, 4), range(4, 8)):
            part = aug.draw(step, pos, [lengths[p] for p in pos])
            assert part.speed == whole.speed and (part.taps is None) == (whole.taps is None)
            assert part.taps is None or np.array_equal(part.taps, whole.taps)
            for j, p in enumerate(pos):
                assert part.out_lens[j] == whole.out_lens[p] and part.counts[j] == whole.counts[p]
                assert np.array_equal(part.chunks[j], whole.chunks[p])
        # a chunk lies inside the utterance when the utterance is longer than the chunk
        for b in range(8):
            for s, e in whole.chunks[b, :whole.counts[b]]:
                assert 0 <= s and 1000 <= e - s <= 2000 and (e <= whole.out_lens[b] or s == 0)
        seen.add((whole.speed, len(whole.freqs), tuple(whole.counts)))
    assert len(seen) > 6  # steps differ
    assert {s for s, _, _ in seen} == {95, 100, 105}
    a, b = aug.draw(3, range(8), lengths), aug.draw(4, range(8), lengths)
    assert not np.array_equal(a.chunks, b.chunks)
    other = TimeDomainSpecAugmentDevice(seed=8).draw(3, range(8), lengths)
    assert not np.array_equal(a.chunks, other.chunks)


def test_skipped_stages_still_consume_their_draws():
    from ssak_amd.augment import TimeDomainSpecAugmentDevice
    lengths = [16000, 9000, 20001, 5000]
    full = TimeDomainSpecAugmentDevice(seed=11)
    no_freq = TimeDomainSpecAugmentDevice(seed=11, drop_freq_prob=0.0)
    no_speed = TimeDomainSpecAugmentDevice(seed=11, perturb_prob=0.0)
    no_chunk = TimeDomainSpecAugmentDevice(seed=11, drop_chunk_prob=0.0)
    any_freq = False
    for step in range(1, 9):
        t = full.draw(step, range(4), lengths)
        any_freq |= t.taps is not None
        nf = no_freq.draw(step, range(4), lengths)
        assert nf.taps is None and nf.speed == t.speed
        assert np.array_equal(nf.chunks, t.chunks) and np.array_equal(nf.counts, t.counts)
        _check(nf, R.draw(11, step, range(4), lengths, drop_freq_prob=0.0))
        ns = no_speed.draw(step, range(4), lengths)
        assert ns.speed == 100 and ns.speed_index is None and list(ns.out_lens) == lengths
        assert (ns.taps is None) == (t.taps is None) and (t.taps is None or np.array_equal(ns.taps, t.taps))
        _check(ns, R.draw(11, step, range(4), lengths, perturb_prob=0.0))
        nc = no_chunk.draw(step, range(4), lengths)
        assert not nc.counts.any() and nc.speed == t.speed
        _check(nc, R.draw(11, step, range(4), lengths, drop_chunk_prob=0.0))
    assert any_freq


def test_other_count_and_length_ranges():
    from ssak_amd.augment import TimeDomainSpecAugmentDevice
    aug = TimeDomainSpecAugmentDevice(seed=5, speeds=[90, 110], drop_freq_count_low=2, drop_freq_count_high=2, drop_chunk_count_low=3,
                                      drop_chunk_count_high=7, drop_chunk_length_low=10, drop_chunk_length_high=20)
    for step in (1, 2, 3):
        t = aug.draw(step, [5, 9], [4000, 15])
        _check(t, R.draw(5, step, [5, 9], [4000, 15], speeds=(90, 110), freq_count=(2, 2), chunk_count=(3, 7), chunk_length=(10, 20)))
        assert t.chunks.shape == (2, 7, 2) and len(t.freqs) == 2 and (3 <= t.counts).all()


# ------------------------------------------------------------------ yaml
def _hp(tmp_path, text, overrides=None):
    from ssak_amd.train_speechbrain import load_hparams
    p = tmp_path / "hp.yaml"
    p.write_text("seed: 1234\nlr: 1.0\n" + text)
    return load_hparams(str(p), overrides or {})


def test_yaml_finetune_block_builds_the_time_domain_class(tmp_path):
    from ssak_amd.augment import TimeDomainSpecAugmentDevice
    from ssak_amd.train_speechbrain import select_augmentation
    hp = _hp(tmp_path, FINETUNE_BLOCK)
    assert hp["augmentation"] == {"sample_rate": 16000, "speeds": [95, 100, 105]}  # still equal to the plain mapping
    cls, kw = select_augmentation(hp, seed=1234)
    assert cls is TimeDomainSpecAugmentDevice
    aug = cls(**kw)
    assert aug.speeds == [95, 100, 105] and aug.sample_rate == 16000 and aug.seed == 1234
    assert aug.chunk_count == (0, 5) and aug.chunk_length == (1000, 2000) and aug.freq_count == (0, 3)
    hp = _hp(tmp_path, FINETUNE_BLOCK + "    drop_chunk_count_high: 2\n    perturb_prob: 0.5\n")
    aug = (lambda c, k: c(**k))(*select_augmentation(hp, seed=1))
    assert aug.chunk_count == (0, 2) and aug.perturb_prob == 0.5 and aug.max_chunks == 2


def test_yaml_speech_augment_block_selects_the_other_class(tmp_path):
    from ssak_amd.augment import SpeechAugmentDevice
    from ssak_amd.train_speechbrain import select_augmentation
    cls, kw = select_augmentation(_hp(tmp_path, SPEECH_AUGMENT_BLOCK), seed=3)
    assert cls is SpeechAugmentDevice
    assert kw == {"noise_dir": "/corpus/noise", "rir_arg": "/corpus/rirs/[small/rir_list,large/rir_list]", "sample_rate": 16000, "seed": 3}
    # apply_prob is not honoured: anything but 1 is refused, the reference class's default (0.5) included
    with pytest.raises(ValueError, match="apply_prob"):
        select_augmentation(_hp(tmp_path, SPEECH_AUGMENT_BLOCK.replace("apply_prob: 1", "apply_prob: 0.5")))
    with pytest.raises(ValueError, match="apply_prob"):
        select_augmentation(_hp(tmp_path, SPEECH_AUGMENT_BLOCK.replace("    apply_prob: 1\n", "")))


def test_yaml_without_augmentation_or_with_none(tmp_path):
    from ssak_amd.train_speechbrain import select_augmentation
    assert select_augmentation(_hp(tmp_path, "sample_rate: 16000\n")) is None
    assert select_augmentation(_hp(tmp_path, "augmentation: null\n")) is None
    assert select_augmentation(_hp(tmp_path, FINETUNE_BLOCK, {"augmentation": "none"})) is None
    assert select_augmentation(_hp(tmp_path, "sample_rate: 16000\n", {"augmentation": "none"})) is None


def test_yaml_unknown_class_and_unsupported_arguments_raise(tmp_path):
    from ssak_amd.train_speechbrain import main, select_augmentation
    with pytest.raises(ValueError, match="speechbrain.lobes.augment.SpecAugment"):
        select_augmentation(_hp(tmp_path, "augmentation: !new:speechbrain.lobes.augment.SpecAugment\n    time_warp: True\n"))
    with pytest.raises(ValueError, match="drop_chunk_noise_factor"):
        select_augmentation(_hp(tmp_path, FINETUNE_BLOCK + "    drop_chunk_noise_factor: 0.1\n"))
    with pytest.raises(ValueError, match="frobnicate"):
        select_augmentation(_hp(tmp_path, FINETUNE_BLOCK + "    frobnicate: 1\n"))
    # the command line reports it before it touches a model or a device
    p = tmp_path / "bad.yaml"
    p.write_text("seed: 1\n" + FINETUNE_BLOCK + "    drop_chunk_noise_factor: 0.1\n")
    with pytest.raises(SystemExit, match="drop_chunk_noise_factor"):
        main([str(p), "--base_model=/nonexistent"])
