"""GPU: MMS language adapters -- the adapter layer's closing row kernel against its float64 restatement
(tests/attn_adapter_ref.py, where the bars are derived), the model against transformers' logits for the default load and after
``load_adapter`` of each language (tests/golden/mms_tiny.npz, written by tests/gen_golden_mms.py), the public inference path
with ``language``, and the documented refusals."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attn_adapter_ref as AR  # noqa: E402
import gen_golden_mms as GM  # noqa: E402
import rowwise_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
A = 16


def _dev(a, dt):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).to(dt).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _case(M, H, bf, seed, near_eps=False):
    """Operands in the storage type (activations and W1 / W2 rounded to it; affines and biases fp32).  ``near_eps``: rows of
    spread ~3e-3, where eps decides the LayerNorms' scale."""
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.standard_normal(s)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    res, y = 1.5 * g(M, H) + 0.3, 0.7 * g(M, H)
    if near_eps:
        res, y = 3e-3 * g(M, H) + 1e-3, 2e-3 * g(M, H)
    return dict(y=RR.round_to(y, bf), res=RR.round_to(res, bf), ga=f32(1 + 0.2 * g(H)), ba=f32(0.1 * g(H)),
                w1=RR.round_to(g(A, H) / np.sqrt(H), bf), b1=f32(0.3 * g(A)), w2=RR.round_to(g(H, A) / np.sqrt(A), bf),
                b2=f32(0.1 * g(H)), gn=f32(1 + 0.2 * g(H)), bn=f32(0.1 * g(H)))


def _launch(c, dt, eps_a=1e-5, eps_n=1e-5, use_y=True):
    import ssak_amd.hip as hip
    M, H = c["res"].shape
    t = {k: _dev(c[k], dt if k in ("y", "res", "w1", "w2") else F32) for k in c}
    r_out = torch.full((M, H), float("nan"), dtype=dt, device=DEV)
    out = torch.full((M, H), float("nan"), dtype=dt, device=DEV)
    mean, rstd = torch.full((M,), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    hip.test_attn_adapter_fwd(t["y"] if use_y else None, t["res"], t["ga"], t["ba"], t["w1"], t["b1"], t["w2"], t["b2"], t["gn"], t["bn"],
                              r_out, out, mean, rstd, eps_adapter=eps_a, eps_next=eps_n)
    torch.cuda.synchronize()
    return _host(r_out), _host(out), _host(mean), _host(rstd)


def _check(name, got, ref, bar):
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    err = np.abs(got - ref)
    ratio = float((err / bar).max())
    print(f"{name}: max err / bar = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: {int((err > bar).sum())} of {err.size} outside the bar, worst ratio {ratio:.3f}"
    return ratio


def _check_launch(c, dt, got, eps_a=1e-5, eps_n=1e-5):
    bf = dt == BF
    r2p, out, mean, rstd = got
    kw = {k: c[k] for k in ("y", "res", "ga", "ba", "w1", "b1", "w2", "b2")}
    ref = AR.fused_tail(**c, eps_a=eps_a, eps_n=eps_n)
    ratio = _check("r2'", r2p, ref["r2p"], AR.r2p_bar(**kw, eps_a=eps_a, bf16=bf))
    # the next LayerNorm on what the kernel stored (the LayerNorm forward bar of tests/test_gpu_rowwise.py)
    m_ref, s_ref = RR.ln_stats(r2p, eps_n)
    _check("mean", mean, m_ref, 4e-6 * np.abs(r2p).mean(axis=1) + 1e-30)
    _check("rstd", rstd, s_ref, 1e-5 * s_ref)
    o_ref = AR.ln(r2p, c["gn"], c["bn"], eps_n)
    eps_st = 2.0 ** -8 if bf else 2.0 ** -22
    _check("out", out, o_ref, eps_st * np.abs(o_ref) + 1.2 * AR.ln_floor(r2p, c["gn"], c["bn"], eps_n))
    return ratio


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H", [64, 1024, 1280])
@pytest.mark.parametrize("M", [1, 17, 37])
def test_attn_adapter_kernel(M, H, dt):
    """One launch against float64: row tails (M = 1, 17, 37 against the 16-row tile, more than one workgroup), column tails
    (H = 64: a quarter of a wave's chunks; 1280: no multiple of 256), both storage types."""
    c = _case(M, H, dt == BF, seed=1000 * M + H)
    _check_launch(c, dt, _launch(c, dt))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_attn_adapter_exact_structure(dt):
    bf = dt == BF
    half_ulp = lambda x: 0.5 * (RR.bf16_ulp(x) if bf else 2.0 ** -23 * np.abs(x)) + 2 * AR.U * np.abs(x) + 1e-30
    c = _case(37, 1280, bf, seed=5)
    # W2 = 0, b2 = 0: the adapter adds nothing, r2' is r2 up to the store's rounding
    z = dict(c, w2=0 * c["w2"], b2=0 * c["b2"])
    r2p = _launch(z, dt)[0]
    r2 = z["y"] + z["res"]
    assert (np.abs(r2p - r2) <= half_ulp(r2)).all()
    # b1 very negative: every ReLU is off, r2' = r2 + b2
    off = dict(c, b1=c["b1"] - 1e4)
    r2p = _launch(off, dt)[0]
    want = r2 + off["b2"]
    assert (np.abs(r2p - want) <= half_ulp(want) + 2 * AR.U * (np.abs(r2) + np.abs(off["b2"]))).all()
    # y = NULL reads r2 from res alone
    one = dict(c, y=0 * c["y"])
    a, b = _launch(one, dt), _launch(one, dt, use_y=False)
    assert all((p == q).all() for p, q in zip(a, b))


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_attn_adapter_eps_is_an_argument(dt):
    """eps_adapter = 1e-2 on rows of spread ~3e-3 (variance near 1e-5) changes the adapter LayerNorm's scale many times over, and
    eps_next = 1e-3 moves the next LayerNorm's rstd (r2' has variance ~0.08 once b2 and the adapter's output are added: the shift
    is 1e-3 / (2 * 0.08) ~ 0.6 %) by hundreds of times its 1e-5 relative bar: a kernel with 1e-5 built in for either fails the
    checks above.  The two assertions below show that on this data: the values for eps 1e-5 lie outside the bars."""
    c = _case(17, 1024, dt == BF, seed=11, near_eps=True)
    got = _launch(c, dt, eps_a=1e-2, eps_n=1e-3)
    _check_launch(c, dt, got, eps_a=1e-2, eps_n=1e-3)
    base = AR.fused_tail(**c)  # eps 1e-5 in both
    kw = {k: c[k] for k in ("y", "res", "ga", "ba", "w1", "b1", "w2", "b2")}
    assert (np.abs(got[0] - base["r2p"]) > AR.r2p_bar(**kw, bf16=dt == BF)).mean() > 0.5
    shift = np.abs(got[3] / RR.ln_stats(got[0], 1e-5)[1] - 1)
    print(f"rstd of eps_next = 1e-3 against that of 1e-5: relative shift {shift.min():.2e} .. {shift.max():.2e} (bar 1e-5)")
    assert shift.min() > 100 * 1e-5  # (the first version asked for 1e-2, more than this data's 0.6 %: the test's mistake, not the kernel's)


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "mms_tiny.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def folder(golden, tmp_path_factory):
    return GM.write_folder(golden, str(tmp_path_factory.mktemp("mms_tiny")))


def _load(folder, exact):
    from ssak_amd.checkpoint import load_pretrained
    model, tok = load_pretrained(folder, device=DEV)
    if exact:
        from ssak_amd.model import Wav2Vec2ForCTC
        ex = Wav2Vec2ForCTC(model.config, device=DEV, exact=True)
        ex.load_state_dict(model.state_dict())
        ex.name_or_path = folder
        model = ex
    return model.eval(), tok


def _logits(model, golden):
    x = torch.from_numpy(np.array(golden["x"]))
    out = model(x, lengths=torch.from_numpy(np.array(golden["lens"]))).logits.float().cpu().numpy()
    fl = np.full(out.shape[0], out.shape[1])  # every frame, those of the shorter utterance's padding included
    return out, fl


def _valid(a, fl):
    return np.concatenate([a[b, :fl[b]].reshape(-1) for b in range(len(fl))])


def test_model_matches_transformers_exact(golden, folder):
    """fp32-exact mode, the project's exact-mode bar (2e-4 absolute on the logits): the default load, each language after
    load_adapter -- fra changes the head's size, to 21, padded to 24 inside the engine -- and back."""
    model, _ = _load(folder, exact=True)
    assert model.config.adapter_attn_dim == 16 and any("adapter_layer.linear_1.weight" in n for n in model.layout)
    for step, key in (("default", "logits_default"), ("fra", "logits_fra"), ("eng", "logits_eng"), ("fra", "logits_fra")):
        if step != "default":
            model.load_adapter(step)
        got, fl = _logits(model, golden)
        ref = np.array(golden[key])
        assert got.shape == ref.shape, (step, got.shape, ref.shape)
        err = np.abs(_valid(got, fl) - _valid(ref, fl)).max()
        print(f"exact {step}: max abs err {err:.2e}")
        assert err < 2e-4, (step, err)
    h = model._h
    model.load_adapter("fra")  # loaded already: nothing happens
    assert model._h is h


def test_model_matches_transformers_bf16(golden, folder):
    """The bf16 engine at the project's bf16 bar: relative L2 2e-2."""
    model, _ = _load(folder, exact=False)
    for step, key in (("default", "logits_default"), ("fra", "logits_fra"), ("eng", "logits_eng")):
        if step != "default":
            model.load_adapter(step)
        got, fl = _logits(model, golden)
        g, r = _valid(got, fl), _valid(np.array(golden[key]), fl)
        rel = np.linalg.norm(g - r) / np.linalg.norm(r)
        print(f"bf16 {step}: rel L2 {rel:.2e}")
        assert rel < 2e-2, (step, rel)


def test_bin_adapter_loads_like_safetensors(golden, folder, tmp_path):
    other = GM.write_folder(golden, str(tmp_path / "bin"), bin_for=("fra",))
    assert os.path.isfile(os.path.join(other, "adapter.fra.bin")) and not os.path.exists(os.path.join(other, "adapter.fra.safetensors"))
    a, _ = _load(folder, exact=True)
    b, _ = _load(other, exact=True)
    a.load_adapter("fra")
    b.load_adapter("fra")
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert (_logits(a, golden)[0] == _logits(b, golden)[0]).all()


def test_state_dict_round_trips_the_adapter_tensors(golden, folder, tmp_path):
    from ssak_amd.checkpoint import load_pretrained, save_pretrained
    model, tok = _load(folder, exact=False)
    model.load_adapter("fra")
    tok.set_target_lang("fra")
    save_pretrained(model, tok, str(tmp_path / "saved"))
    again, tok2 = load_pretrained(str(tmp_path / "saved"), device=DEV)
    assert tok2.target_lang == "fra" and tok2.languages == ["eng", "fra"] and again.config.vocab_size == 21
    sa, sb = model.state_dict(), again.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    for k in golden.files:
        if k.startswith("a/fra/"):
            assert torch.equal(sa[k[len("a/fra/"):]], torch.from_numpy(np.array(golden[k]))), k


# ------------------------------------------------------------------------------------------------ the public path
def _write_wavs(golden, d):
    """The fixture's two waveforms as 16-bit PCM files (they are values PCM holds exactly: load_audio returns them unchanged)."""
    paths = []
    for i in range(2):
        p = os.path.join(d, f"utt{i}.wav")
        pcm = np.clip(np.round(np.array(golden[f"wave{i}"]) * 32768.0), -32768, 32767).astype("<i2")
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
        paths.append(p)
    return paths


def test_transformers_infer_with_language(golden, folder, tmp_path, monkeypatch):
    """The public path on a folder and .wav files, in the fp32-exact mode (SSAK_EXACT=1): transcripts equal transformers'."""
    from ssak_amd.infer import transformers_infer
    monkeypatch.setenv("SSAK_EXACT", "1")
    texts = json.loads(str(golden["texts_json"]))
    wavs = _write_wavs(golden, str(tmp_path))
    assert list(transformers_infer(folder, wavs, batch_size=2, language="fr")) == texts["fra"]  # unique prefix
    assert list(transformers_infer(folder, wavs, batch_size=2)) == texts[str(golden["default_lang"])]
    assert list(transformers_infer(folder, wavs, batch_size=2, language="eng")) == texts["eng"]
    with pytest.raises(ValueError, match="not in"):
        list(transformers_infer(folder, wavs, language="deu"))


def test_cli_language_in_a_child_process(golden, folder, tmp_path):
    paths = _write_wavs(golden, str(tmp_path))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SSAK_EXACT="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "ssak_amd.infer", *paths, "--model", folder, "--language", "fra",
                        "--batch_size", "2"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines() == json.loads(str(golden["texts_json"]))["fra"]


def test_arpa_sees_the_selected_language(golden, folder, tmp_path, monkeypatch):
    """With --arpa and a language the LM's label table is built over that language's vocabulary."""
    from ssak_amd import lm as lm_mod
    from ssak_amd.infer import transformers_infer
    seen = {}
    real = lm_mod.load_arpa

    def spy(path, tok, device):
        seen["vocab"], seen["lang"] = list(tok.vocab), tok.target_lang
        return real(path, tok, device)

    monkeypatch.setattr(lm_mod, "load_arpa", spy)
    monkeypatch.setenv("SSAK_EXACT", "1")
    out = list(transformers_infer(folder, _write_wavs(golden, str(tmp_path)), batch_size=2, language="fra",
                                  arpa_path=os.path.join(HERE, "golden", "lm_tiny.arpa")))
    assert seen["lang"] == "fra" and seen["vocab"] == GM.LANGS["fra"] and len(out) == 2


# ------------------------------------------------------------------------------------------------ refusals
def test_training_is_refused(golden, folder):
    model, _ = _load(folder, exact=False)
    x = torch.from_numpy(np.array(golden["x"]))
    with pytest.raises(ValueError, match="inference only: training is not implemented"):
        model.train()(x, lengths=torch.from_numpy(np.array(golden["lens"])))
    from ssak_amd import train
    with pytest.raises(NotImplementedError, match="inference only: training is not implemented"):
        train.main(["no_train_folder", "no_valid_folder", "--base_model", folder])  # refused right after parsing: no data is read


def test_post_ln_with_adapter_is_refused_at_create(golden):
    import dataclasses
    from ssak_amd.config import Wav2Vec2Config
    from ssak_amd.model import Wav2Vec2ForCTC
    cfg = Wav2Vec2Config.from_hf_dict(json.loads(str(golden["config_json"])))
    with pytest.raises(ValueError, match="post-LN encoder layer of transformers has no adapter"):
        Wav2Vec2ForCTC(dataclasses.replace(cfg, do_stable_layer_norm=False), device=DEV)
    with pytest.raises(ValueError, match="supported values: adapter_attn_dim 16"):
        Wav2Vec2ForCTC(dataclasses.replace(cfg, adapter_attn_dim=32), device=DEV)
