"""GPU: Whisper fine-tuning composed -- WhisperSeq2Seq.forward_train / backward / save_pretrained and WhisperAdamW
(ssak_amd/whisper_train.py) on the tiny golden model (D 128, 2 heads, 2 layers, V 127, B 3, L 12, S 50, encoder lengths 50 / 50 / 23)
against the float64 restatement tests/whisper_train_ref.py (itself held to transformers by tests/test_whisper_train_ref.py).

Bars are measured, not chosen (the method of ``cpu_bars`` in tests/test_gpu_whisper_decoder.py): on the CPU the restatement is
evaluated once in float64 and once with the device's storage roundings (bf16 activations, residual stream, P into its products, and
the gradients of all of them: dS, dlogits, the activation gradients); a tensor's bar is 4 x the relative L2 distance of the two,
and never more than the project's bf16 gradient bar, 6e-2.  Every test prints what it measured before it asserts.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_train_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAD_BAR = 6e-2  # README "What the parity bars mean": the bf16 gradient bar, relative L2
PRE = "model.decoder."


@pytest.fixture(scope="module")
def golden():
    g = np.load(G.GOLDEN)
    return dict(g=g, w={k[2:]: WR.bf16_from_bits(g[k]) for k in g.files if k.startswith("w/")}, enc=WR.bf16_from_bits(g["enc"]),
                labels=WR.shifted_targets(g["tokens"], g["lens"]), enc_lens=[int(v) for v in g["enc_lens"]])


@pytest.fixture(scope="module")
def folder(golden, tmp_path_factory):
    return G.write_folder(golden["g"], str(tmp_path_factory.mktemp("whisper_train_tiny")))


@pytest.fixture(scope="module")
def ref(golden):
    """(loss, grads, d_enc) of the restatement in float64 and with the device's storage roundings."""
    a = golden
    out = {key: TR.decoder_loss_and_grads(a["w"], G.NH, G.LAYERS, a["enc"], a["labels"], a["enc_lens"], G.EOT, G.SOT, storage=st)
           for key, st in (("f64", False), ("dev", True))}
    return out


def load(folder, **kw):
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq
    return WhisperSeq2Seq.from_pretrained(folder, **kw)


def dev_enc(golden):
    return torch.from_numpy(golden["enc"].astype(np.float32)).to(torch.bfloat16).to(DEV)


def dec_grads_by_name(m):
    torch.cuda.synchronize()
    return {n: m.dec_grad(n).double().cpu().numpy() for n in m.layout}


def check_grads(name, got, want, dev, bar_cap=GRAD_BAR):
    """rel L2 of every tensor against float64 within min(4 x the measured storage distance, the bf16 gradient bar)."""
    worst = ("", 0.0)
    for n, w in want.items():
        d = TR.rel_l2(dev[n], w)
        bar = min(4 * d, bar_cap)
        e = TR.rel_l2(got[n], w)
        print(f"{name} {n}: rel L2 {e:.3e}, measured storage distance {d:.3e}, bar {bar:.3e}, err/bar {e / bar:.3f}")
        if e / bar > worst[1]:
            worst = (n, e / bar)
    print(f"{name}: worst err/bar {worst[1]:.3f} ({worst[0]})")
    for n, w in want.items():
        assert TR.rel_l2(got[n], w) <= min(4 * TR.rel_l2(dev[n], w), bar_cap), n


def test_loss_and_decoder_gradients(folder, golden, ref):
    m = load(folder)
    loss = m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"])
    assert loss.dtype == torch.float32 and loss.is_cuda
    d_enc = m.backward()
    got_loss = float(loss.item())
    want = float(golden["g"]["hf_batch_loss"])
    d = abs(ref["dev"][0] - ref["f64"][0])
    print(f"loss {got_loss:.6f}, transformers {want:.6f}: err {abs(got_loss - want):.3e}, measured storage distance {d:.3e}, bar {4 * d:.3e}")
    assert abs(ref["f64"][0] - want) <= 1e-12
    assert abs(got_loss - want) <= 4 * d
    grads = dec_grads_by_name(m)
    V = G.V
    E = PRE + "embed_tokens.weight"
    assert (grads[E][V:] == 0).all(), "the vocabulary's padding rows get no gradient"
    grads[E] = grads[E][:V]
    for n in list(grads):
        if n.endswith("k_proj.bias"):
            assert (grads.pop(n) == 0).all(), "the synthetic k_proj.bias slot gets no gradient"
    assert set(grads) == set(ref["f64"][1])
    check_grads("decoder", grads, ref["f64"][1], ref["dev"][1])
    de = d_enc.double().cpu().numpy()
    check_grads("d_enc", {"d_enc": de}, {"d_enc": ref["f64"][2]}, {"d_enc": ref["dev"][2]})
    assert (de[2, golden["enc_lens"][2]:] == 0).all(), "frames past enc_lens get no gradient"
    # the same step again: the same bits
    loss2 = m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"])
    m.backward()
    torch.cuda.synchronize()
    g2 = m.dec_grads.clone()
    m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"])
    m.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(g2.view(torch.int32), m.dec_grads.view(torch.int32)), "two runs differ"


def test_row_chunk_does_not_change_the_gradients(folder, golden):
    """row_chunk = 5 does not divide the 36 rows: 8 chunks against one.  What chunking changes is counted, not guessed:
    * a logit is one K = 128 dot product of its own row, summed in the same order whatever the number of rows in the product, and the
      loss is one sum over the concatenated per-row log-probabilities: loss, dlogits, dX and with them EVERY gradient downstream
      (all layers, the position table, d_enc) must be bit-identical;
    * only the tied embedding's gradient is summed differently: dE = sum over chunks of dlogits^T X, 8 `accumulate` passes of at
      most 5 terms each against one product of 36 terms.  Any order of summing n fp32 terms is within (n - 1) u sum |terms| of the
      exact sum; the two runs differ by at most the sum of their errors, (35 + 36 + 8) u mag with mag = |dlogits|^T |X| taken from the
      device's own bf16 operands, plus the gathered rows' `+=` in each run (2 u |dE|).  Per element."""
    from ssak_amd import hip
    u = 2.0 ** -24
    m = load(folder)
    out = []
    for chunk in (256, 5):
        m.row_chunk = chunk
        loss = m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"])
        if chunk == 256:
            xf, targets, n_scored = m._train["ln_f"][1], m._train["targets"], m._train["n_scored"]
            dl = hip.dec_ce_bwd(m._project(xf, xf.shape[0]), G.V, targets, 1.0 / n_scored, want_loss=False)[0]
            mag = (dl.double().abs().T @ xf.double().abs()).cpu().numpy()
        d_enc = m.backward()
        torch.cuda.synchronize()
        out.append((loss.clone(), {n: m.dec_grad(n).clone() for n in m.layout}, d_enc.clone()))
    (la, ga, ea), (lb, gb, eb) = out
    E = PRE + "embed_tokens.weight"
    differing = [n for n in ga if not torch.equal(ga[n].view(torch.int32), gb[n].view(torch.int32))]
    a, b = ga[E].double().cpu().numpy(), gb[E].double().cpu().numpy()
    bar = (35 + 36 + 8) * u * mag + 2 * u * np.abs(a)
    err = np.abs(a - b)
    print(f"row_chunk 5 vs one chunk: loss {float(la):.7f} / {float(lb):.7f}; tensors that differ by a bit: {differing}; embed_tokens rel L2 "
          f"{TR.rel_l2(b, a):.3e}, {int((err > 0).sum())} of {err.size} elements differ, worst err/bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
    assert torch.equal(la, lb), "the loss depends on row_chunk"
    assert torch.equal(ea.view(torch.int32), eb.view(torch.int32)), "d_enc depends on row_chunk"
    assert set(differing) <= {E}, differing
    assert (err <= bar).all()


def hf_whole_model(folder, storage):
    """transformers' WhisperForConditionalGeneration in float64 with the folder's weights; ``storage``: every Linear / Conv1d /
    LayerNorm / Embedding output rounded to bf16 on the way forward and its gradient on the way back (the device's stored tensors)."""
    from safetensors.torch import load_file
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    with open(os.path.join(folder, "config.json")) as f:
        cfg = {k: v for k, v in json.load(f).items() if k not in ("architectures", "model_type")}
    model = WhisperForConditionalGeneration(WhisperConfig(**cfg)).double().eval()
    sd = {k: v.double() for k, v in load_file(os.path.join(folder, "model.safetensors")).items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    own = model.state_dict()
    model.load_state_dict({k: sd.get(k, own[k]) for k in own})
    if storage:
        rnd = TR._make_round()
        for mod in model.modules():
            if isinstance(mod, (torch.nn.Linear, torch.nn.Conv1d, torch.nn.LayerNorm, torch.nn.Embedding)):
                mod.register_forward_hook(lambda _m, _i, out: rnd(out, True, True))
    return model


def test_encoder_gradients_through_backward_hidden(folder, golden, ref):
    """Input features [3, 80, 100] through the 1-layer tiny encoder: the first test of backward_hidden on the Whisper topology.
    Against transformers in float64 on the whole model when it imports; otherwise the engine's own backward_hidden is fed the
    restatement's d_enc and must reproduce the gradients of the composed step (the decoder's d_enc within its bar)."""
    m = load(folder)
    rng = np.random.default_rng(3)
    feats = rng.standard_normal((G.B, G.MELS, 2 * G.S)).astype(np.float32)
    labels = golden["labels"]
    loss = m.forward_train(torch.from_numpy(feats), labels)
    m.backward()
    torch.cuda.synchronize()
    enc = m.encoder
    got = {"model." + n: enc.grad(n).double().cpu().numpy() for n in enc.layout if not n.startswith("ctc_head.") and not n.endswith("k_proj.bias")}
    try:
        import transformers  # noqa: F401
    except ImportError:
        # the engine's own backward_hidden fed the restatement's d_enc of the encoder output it produced; the encoder's backward is
        # linear in d_enc, so the composed step may differ from it by the decoder's measured d_enc distance (x 4)
        enc.train()
        hidden, _ = enc.forward_hidden(torch.from_numpy(feats))
        _, _, d_enc = TR.decoder_loss_and_grads(golden["w"], G.NH, G.LAYERS, hidden.double().cpu().numpy(), labels, None, G.EOT, G.SOT)
        enc.backward_hidden(torch.from_numpy(d_enc.astype(np.float32)).to(torch.bfloat16).to(DEV))
        enc.eval()
        torch.cuda.synchronize()
        bar = min(4 * TR.rel_l2(ref["dev"][2], ref["f64"][2]), GRAD_BAR)
        for n in got:
            own = enc.grad(n[len("model."):]).double().cpu().numpy()
            if np.abs(own).max() > 0:
                print(f"encoder {n}: rel L2 against backward_hidden on the restatement's d_enc {TR.rel_l2(got[n], own):.3e}, bar {bar:.3e}")
                assert TR.rel_l2(got[n], own) <= bar, n
        return
    res = {}
    for key, st in (("f64", False), ("dev", True)):
        hf = hf_whole_model(folder, st)
        out = hf(input_features=torch.from_numpy(feats).double(), labels=torch.from_numpy(labels.astype(np.int64)))
        out.loss.backward()
        res[key] = (float(out.loss), {n: p.grad.numpy() for n, p in hf.named_parameters() if n.startswith("model.encoder.") and p.grad is not None})
    d = abs(res["dev"][0] - res["f64"][0])
    print(f"loss through the encoder {float(loss.item()):.6f}, transformers {res['f64'][0]:.6f}, measured storage distance {d:.3e}")
    assert abs(float(loss.item()) - res["f64"][0]) <= max(4 * d, 0.0)
    want = res["f64"][1]
    assert set(want) <= set(got)
    check_grads("encoder", {n: got[n] for n in want}, want, res["dev"][1])


def test_twenty_step_curve_follows_the_reference(folder, golden):
    """One fixed batch, AdamW (lr 1e-3, no warm-up, weight decay 0.01, clip 1.0), 20 steps on the stored encoder output.  Reference:
    the float64 restatement under torch.optim.AdamW.  Bar: 4 x the largest distance between that curve and the same reference
    with its weights re-rounded to bf16 for each forward (the engine's shadow)."""
    from ssak_amd.trainer import linear_warmup_lr
    from ssak_amd.whisper_train import WhisperAdamW
    steps, lr, total = 20, 1e-3, 1000
    a = golden
    curves = {}
    for key, rw in (("f64", False), ("shadow", True)):
        params = {k: torch.tensor(v, requires_grad=True) for k, v in a["w"].items()}
        decay = [p for n, p in params.items() if "layer_norm" not in n and "bias" not in n]
        rest = [p for n, p in params.items() if "layer_norm" in n or "bias" in n]
        opt = torch.optim.AdamW([{"params": decay, "weight_decay": 0.01}, {"params": rest, "weight_decay": 0.0}], lr=lr, betas=(0.9, 0.999), eps=1e-8)
        curve = []
        for i in range(steps):
            for gr in opt.param_groups:
                gr["lr"] = linear_warmup_lr(lr, i, 0, total)
            opt.zero_grad()
            loss, _ = TR.decoder_loss_and_grads(None, G.NH, G.LAYERS, a["enc"], a["labels"], a["enc_lens"], G.EOT, G.SOT, round_weights=rw, params=params)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
            opt.step()
            curve.append(float(loss.detach()))
        curves[key] = np.array(curve)
    m = load(folder, freeze_encoder=True)
    opt = WhisperAdamW(m, lr=lr, weight_decay=0.01, warmup_steps=0, total_steps=total, max_grad_norm=1.0)
    enc = dev_enc(golden)
    losses = []
    for i in range(steps):
        losses.append(m.forward_train(enc, a["labels"], a["enc_lens"]))
        m.backward()
        opt.step()
    dev = torch.cat(losses).double().cpu().numpy()
    d = float(np.abs(curves["shadow"] - curves["f64"]).max())
    e = float(np.abs(dev - curves["f64"]).max())
    print("step  device      float64     float64 + bf16 shadow")
    for i in range(steps):
        print(f"{i:4d}  {dev[i]:.6f}  {curves['f64'][i]:.6f}  {curves['shadow'][i]:.6f}")
    print(f"20-step curve: max |device - float64| {e:.3e}, measured distance to the shadowed reference {d:.3e}, bar {4 * d:.3e}, err/bar {e / (4 * d):.3f}")
    assert dev[-1] < 0.5 * dev[0] and curves["f64"][-1] < 0.5 * curves["f64"][0]
    assert e <= 4 * d


def test_freeze_encoder_leaves_the_encoder_alone(folder, golden):
    from ssak_amd.whisper_train import WhisperAdamW
    m = load(folder, freeze_encoder=True)
    before_p, before_s = m.encoder.params.clone(), m.encoder.shadow.clone()
    dec_before = m.dec_params.clone()
    opt = WhisperAdamW(m, lr=1e-3, warmup_steps=0)
    feats = torch.from_numpy(np.random.default_rng(4).standard_normal((G.B, G.MELS, 2 * G.S)).astype(np.float32))
    m.forward_train(feats, golden["labels"])
    m.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(before_p.view(torch.int32), m.encoder.params.view(torch.int32)) and torch.equal(before_s.view(torch.int16), m.encoder.shadow.view(torch.int16))
    assert not torch.equal(dec_before, m.dec_params), "the decoder did not move"
    assert torch.equal(m.dec_params.to(torch.bfloat16).view(torch.int16), m.dec_shadow.view(torch.int16)), "the bf16 shadow follows the step"


def test_step_moves_the_encoder_and_round_trips_through_a_folder(folder, golden, tmp_path):
    from ssak_amd.whisper_train import WhisperAdamW
    m = load(folder)
    enc_before = m.encoder.params.clone()
    opt = WhisperAdamW(m, lr=1e-3, warmup_steps=0)
    feats = torch.from_numpy(np.random.default_rng(5).standard_normal((G.B, G.MELS, 2 * G.S)).astype(np.float32))
    m.forward_train(feats, golden["labels"])
    m.backward()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(enc_before, m.encoder.params), "the encoder did not move"
    assert opt.grad_norm() > 0
    k_bias = [n for n in m.layout if n.endswith("k_proj.bias")]
    assert k_bias and all(bool((m.dec_param(n) == 0).all()) for n in k_bias), "a synthetic k_proj.bias slot moved"
    out = m.save_pretrained(str(tmp_path / "ckpt"))
    from safetensors.torch import load_file
    sd = load_file(os.path.join(out, "model.safetensors"))
    assert all(v.dtype == torch.float32 for v in sd.values()) and not any(k.endswith("k_proj.bias") or "ctc_head" in k for k in sd)
    assert sd["model.decoder.embed_tokens.weight"].shape == (G.V, G.D) and torch.equal(sd["proj_out.weight"], sd["model.decoder.embed_tokens.weight"])
    assert os.path.isfile(os.path.join(out, "config.json")) and os.path.isfile(os.path.join(out, "generation_config.json"))
    m2 = load(out)
    torch.cuda.synchronize()
    assert torch.equal(m.dec_params.view(torch.int32), m2.dec_params.view(torch.int32)), "the decoder does not read back bit for bit"
    for n in m.encoder.layout:
        if not n.startswith("ctc_head."):
            assert torch.equal(m.encoder.param(n).view(torch.int32), m2.encoder.param(n).view(torch.int32)), n


def test_refusals(folder, golden, tmp_path):
    m = load(folder)
    enc = dev_enc(golden)
    with pytest.raises(ValueError, match="no scored token"):
        m.forward_train(enc, np.full((G.B, 4), -100))
    with pytest.raises(ValueError, match="vocabulary"):
        m.forward_train(enc, np.full((G.B, 4), G.V))
    with pytest.raises(RuntimeError, match="forward_train"):
        m.backward()
    for name in ("dropout", "attention_dropout", "activation_dropout", "decoder_layerdrop"):
        bad = load(G.write_folder(golden["g"], str(tmp_path / name), config_overrides={name: 0.1}))
        with pytest.raises(ValueError, match=name):
            bad.forward_train(enc, golden["labels"])


def test_training_loop_on_a_synthetic_kaldi_folder(golden, tmp_path):
    """ssak_amd.train_whisper.run_training on four 1 s synthetic utterances with a stub tokenizer: a first validation, three steps
    through the log-mel front end and the full 1500-frame encoder, a validation with a checkpoint that loads, the final model."""
    from ssak_amd.data import load_kaldi
    from ssak_amd.synth import write_kaldi_folder
    from ssak_amd.train_whisper import run_training
    data = str(tmp_path / "kaldi")
    write_kaldi_folder(data, 4, seconds=1.0, seed=11, threads=2)
    utts = load_kaldi(data)
    assert len(utts) == 4
    m = load(G.write_folder(golden["g"], str(tmp_path / "model"), max_source_positions=1500, encoder_layers=1))
    tokenize = lambda text: [G.SOT] + [ord(c) % 90 for c in text[:9]] + [G.EOT]
    out = str(tmp_path / "out")
    recs = run_training(m, utts, utts[:2], tokenize, batch_size=2, learning_rate=1e-3, warmup_steps=0, num_epochs=2, max_steps=3, eval_steps=3,
                        output_dir=out, detokenize=lambda ids: " ".join(chr(97 + i % 26) for i in ids), log=lambda rec: print(rec))
    steps = [r for r in recs if "loss" in r]
    evals = [r for r in recs if "eval_loss" in r]
    assert [r["step"] for r in steps] == [1, 2, 3] and all(np.isfinite(r["loss"]) and r["grad_norm"] > 0 for r in steps)
    assert [r["step"] for r in evals] == [0, 3] and evals[0]["eval_tokens"] == 20 and all(np.isfinite(r["eval_loss"]) for r in evals)
    # the WER half: greedy generate() on the encoder output (language detected), the stub's text against the utterance's
    assert all(np.isfinite(r["eval_wer"]) and r["eval_wer"] > 0 for r in evals)
    assert evals[1]["eval_loss"] < evals[0]["eval_loss"], "three steps at lr 1e-3 on a set that holds the validation utterances lower its loss"
    assert os.path.isfile(os.path.join(out, "checkpoint-3", "model.safetensors")) and os.path.isfile(os.path.join(out, "model.safetensors"))
    m2 = load(os.path.join(out, "checkpoint-3"))
    assert torch.equal(m.dec_params.view(torch.int32), m2.dec_params.view(torch.int32))


def test_save_pretrained_of_a_model_built_from_a_configuration(golden, tmp_path):
    """No source folder: config.json and generation_config.json are written from the configuration object, and from_pretrained reads
    the same configuration (the generation ids, the language and task tables) and the same parameters back."""
    import dataclasses
    from ssak_amd.whisper_seq2seq import WhisperSeq2Seq, WhisperSeq2SeqConfig
    g = golden["g"]
    gen = json.loads(str(g["generation_config_json"]))
    extra = {k: gen[k] for k in ("decoder_start_token_id", "eos_token_id", "pad_token_id", "task_to_id", "no_timestamps_token_id")}
    cfg = WhisperSeq2SeqConfig.from_hf_dict(json.loads(str(g["config_json"])), lang_to_id={k[2:-2]: v for k, v in gen["lang_to_id"].items()},
                                            suppress_tokens=[1, 2], begin_suppress_tokens=[3], **extra)
    m = WhisperSeq2Seq(cfg)
    m.load_decoder_state_dict({k[2:]: torch.from_numpy(WR.bf16_from_bits(g[k]).astype(np.float32)) for k in g.files if k.startswith("w/")})
    m.encoder.params.copy_(torch.randn(m.encoder.params.numel(), generator=torch.Generator().manual_seed(2)).to(DEV) * 0.05)
    for n in m.encoder.layout:
        if n.startswith("ctc_head.") or n.endswith("k_proj.bias"):
            m.encoder.param(n).zero_()
    assert m.name_or_path is None
    out = m.save_pretrained(str(tmp_path / "from_config"))
    m2 = load(out)
    assert dataclasses.asdict(m2.config) == dataclasses.asdict(cfg)
    assert m2.lang_codes == list(G.LANGS)
    torch.cuda.synchronize()
    assert torch.equal(m.dec_params.view(torch.int32), m2.dec_params.view(torch.int32))
    for n in m.encoder.layout:
        if not n.startswith("ctc_head."):
            assert torch.equal(m.encoder.param(n).view(torch.int32), m2.encoder.param(n).view(torch.int32)), n


def test_a_step_on_an_encoder_output_leaves_the_encoder_alone(folder, golden):
    """forward_train on an encoder output the caller computed, without freeze_encoder: backward fills no encoder gradient, and
    WhisperAdamW must neither decay nor step the encoder nor count its stale gradients into the clip norm."""
    from ssak_amd.whisper_train import WhisperAdamW
    m = load(folder)
    opt = WhisperAdamW(m, lr=1e-3, weight_decay=0.01, warmup_steps=0)
    feats = torch.from_numpy(np.random.default_rng(6).standard_normal((G.B, G.MELS, 2 * G.S)).astype(np.float32))
    m.forward_train(feats, golden["labels"])
    m.backward()
    opt.step()  # a whole step: the encoder moves and its gradient buffer is left filled
    torch.cuda.synchronize()
    assert m.encoder_grads_ready and opt.half_steps == [1, 1]
    before = m.encoder.params.clone()
    m.forward_train(dev_enc(golden), golden["labels"], golden["enc_lens"])
    m.backward()
    opt.step()
    torch.cuda.synchronize()
    assert not m.encoder_grads_ready and opt.half_steps == [1, 2]
    assert torch.equal(before.view(torch.int32), m.encoder.params.view(torch.int32)), "the encoder moved on stale gradients"
    dec_norm = float(m.dec_grads.double().norm())
    print(f"clip norm {opt.grad_norm():.6f}, decoder gradient norm {dec_norm:.6f}")
    assert abs(opt.grad_norm() - dec_norm) <= 1e-5 * dec_norm, "the stale encoder gradients entered the clip norm"
