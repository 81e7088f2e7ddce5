"""CPU: the float64 restatement of the Whisper decoder's training arithmetic (tests/whisper_train_ref.py) against transformers in
float64 on the golden tiny model, and the host helpers of the training path (shift_tokens_right, the embedding backward's CSR, the
weight-decay grouping of decoder names)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_whisper_dec as G  # noqa: E402
import whisper_decoder_ref as WR  # noqa: E402
import whisper_train_ref as TR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    g = np.load(G.GOLDEN)
    w = {k[2:]: WR.bf16_from_bits(g[k]) for k in g.files if k.startswith("w/")}
    return g, w, WR.bf16_from_bits(g["enc"]), WR.shifted_targets(g["tokens"], g["lens"])


def test_shift_tokens_right_rebuilds_the_golden_inputs(golden):
    g, _, _, labels = golden
    ids = TR.shift_tokens_right(labels, G.EOT, G.SOT)
    for b, n in enumerate(g["lens"]):
        assert (ids[b, :n] == g["tokens"][b, :n]).all() and (ids[b, n:] == G.EOT).all()
    transformers = pytest.importorskip("transformers")
    import torch
    from transformers.models.whisper.modeling_whisper import shift_tokens_right
    assert np.array_equal(shift_tokens_right(torch.from_numpy(labels), G.EOT, G.SOT).numpy(), ids)


def test_restatement_loss_equals_the_golden(golden):
    g, w, enc, labels = golden
    loss, _, _ = TR.decoder_loss_and_grads(w, G.NH, G.LAYERS, enc, labels, g["enc_lens"], G.EOT, G.SOT)
    assert abs(loss - float(g["hf_batch_loss"])) <= 1e-12 * abs(loss)


def test_restatement_gradients_equal_transformers(golden):
    """transformers takes no encoder mask: each utterance runs on its first enc_lens[b] frames, its loss weighted by its token
    count, as the generator does.  Every decoder parameter (the tied embedding through both of its uses) and enc, 1e-9 relative."""
    pytest.importorskip("transformers")
    import torch
    g, w, enc, labels = golden
    loss, grads, d_enc = TR.decoder_loss_and_grads(w, G.NH, G.LAYERS, enc, labels, g["enc_lens"], G.EOT, G.SOT)
    model = G.hf_model(w)
    ids = TR.shift_tokens_right(labels, G.EOT, G.SOT)
    n_all = int((labels >= 0).sum())
    hf_d_enc = np.zeros_like(enc)
    total = 0.0
    for b in range(G.B):
        n_b = int((labels[b] >= 0).sum())
        if n_b == 0:
            continue
        e = torch.tensor(enc[b:b + 1, :g["enc_lens"][b]], requires_grad=True)
        out = model(encoder_outputs=(e,), decoder_input_ids=torch.from_numpy(ids[b:b + 1].astype(np.int64)),
                    labels=torch.from_numpy(labels[b:b + 1].astype(np.int64)))
        part = out.loss * n_b / n_all
        part.backward()
        total += float(part)
        hf_d_enc[b, :g["enc_lens"][b]] = e.grad.numpy()[0]
    assert abs(total - loss) <= 1e-12 * abs(loss)
    hf = dict(model.named_parameters())
    worst = 0.0
    for name, gr in grads.items():
        want = hf[name].grad.numpy()
        worst = max(worst, TR.rel_l2(gr, want))
        assert TR.rel_l2(gr, want) <= 1e-9, name
    assert TR.rel_l2(d_enc, hf_d_enc) <= 1e-9
    assert (d_enc[2, g["enc_lens"][2]:] == 0).all()
    # the embedding's gradient has both uses in it: the projection alone touches every row, the lookup only the ids used
    E = grads["model.decoder.embed_tokens.weight"]
    assert np.abs(E).min() > 0
    print(f"worst relative L2 over {len(grads)} tensors: {worst:.2e}")


def test_per_op_references_agree_with_autograd():
    """attention_bwd, ce_bwd and embed_bwd of whisper_train_ref.py against torch autograd in float64."""
    import torch
    rng = np.random.default_rng(0)
    B, Lq, Lk, D, nh, klens = 2, 5, 7, 128, 2, (7, 3)
    q, k, v, do = (WR.bf16_round(rng.standard_normal((B, n, D))) for n in (Lq, Lk, Lk, Lq))
    for causal, q_offset, kl in ((False, 0, klens), (True, 2, None)):
        ctx = WR.attention(q, k, v, nh, kl, causal, q_offset)
        lse = TR.attention_lse(q, k, nh, kl, causal, q_offset)
        ref, _ = TR.attention_bwd(q, k, v, ctx, lse, do, nh, kl, causal, q_offset)
        tq, tk, tv = (torch.tensor(x, requires_grad=True) for x in (q, k, v))
        outs = []
        for b in range(B):
            vis = torch.from_numpy(np.array(TR._visible(Lq, Lk, Lk if kl is None else kl[b], causal, q_offset)))
            heads = []
            for h in range(nh):
                sl = slice(64 * h, 64 * h + 64)
                s = ((tq[b, :, sl] * 0.125) @ tk[b, :, sl].T).masked_fill(~vis, -np.inf)
                heads.append(torch.softmax(s, -1) @ tv[b, :, sl])
            outs.append(torch.cat(heads, -1))
        torch.stack(outs).backward(torch.tensor(do))
        for name, t in (("dq", tq), ("dk", tk), ("dv", tv)):
            assert np.abs(t.grad.numpy() - ref[name]).max() <= 1e-12, (name, causal)
    x = rng.standard_normal((5, 11)) * 3
    t = np.array([3, -100, 10, 0, -100])
    r = TR.ce_bwd(x, t, 0.5)
    tx = torch.tensor(x, requires_grad=True)
    loss = torch.nn.functional.cross_entropy(tx, torch.from_numpy(t), ignore_index=-100, reduction="sum")
    (0.5 * loss).backward()
    assert np.abs(tx.grad.numpy() - r["dlogits"]).max() <= 1e-13 and abs(float(loss) - r["loss_sum"]) <= 1e-12
    ids = rng.integers(0, 6, (3, 4))
    dh = rng.standard_normal((3, 4, 8))
    E, P = torch.zeros(9, 8, dtype=torch.float64, requires_grad=True), torch.zeros(10, 8, dtype=torch.float64, requires_grad=True)
    (E[torch.from_numpy(ids)] + P[2:6][None]).backward(torch.from_numpy(dh))
    dt, dp, _, _ = TR.embed_bwd(dh, ids, 9, 10, 2)
    assert np.abs(dt - E.grad.numpy()).max() <= 1e-13 and np.abs(dp - P.grad.numpy()).max() <= 1e-13


def test_embed_csr_builder():
    """uniq ascending, each id's rows ascending, every row exactly once."""
    import ssak_amd.hip as hip
    ids = np.array([[5, 2, 5, 9], [2, 2, 0, 5]])
    uniq, offs, rows = hip.dec_embed_csr(ids)
    assert uniq.tolist() == [0, 2, 5, 9] and offs.tolist() == [0, 1, 4, 7, 8]
    assert rows.tolist() == [6, 1, 4, 5, 0, 2, 7, 3]
    assert all(a.dtype == np.int32 for a in (uniq, offs, rows))
    uniq, offs, rows = hip.dec_embed_csr(np.full((3, 4), 7))
    assert uniq.tolist() == [7] and offs.tolist() == [0, 12] and rows.tolist() == list(range(12))


def test_weight_decay_groups_of_decoder_names():
    """HF Trainer decays what is not inside an nn.LayerNorm and has no "bias" in its name: the embeddings and every matrix."""
    from ssak_amd.trainer import hf_decays
    names = G.decoder_param_shapes()
    decayed = {n for n in names if hf_decays(n, None)}
    assert "model.decoder.embed_tokens.weight" in decayed and "model.decoder.embed_positions.weight" in decayed
    assert all(n.endswith(".weight") and "layer_norm" not in n for n in decayed)
    assert {n for n in names if n.endswith("proj.weight") or ".fc" in n and n.endswith("weight")} <= decayed
    assert not any("layer_norm" in n or n.endswith(".bias") for n in decayed)


def test_command_line_refusals(capsys):
    """What the reference's command line offers and this one does not build is refused by name; the defaults are the reference's
    except gradient accumulation (1 here, 16 there)."""
    from ssak_amd.train_whisper import make_labels, parse_args
    base = ["train_dir", "valid_dir", "--base_model", "model_dir"]
    a = parse_args(base)
    assert (a.batch_size, a.batch_size_eval, a.learning_rate, a.weight_decay, a.max_duration, a.max_text_length) == (8, 8, 1e-5, 0.01, 30, 448)
    assert a.gradient_accumulation_steps == 1 and a.lang == "fr" and a.task == "transcribe" and a.warmup_steps is None
    assert parse_args(base + ["--gradient_accumulation_steps", "1", "--batch_size_eval", "2"]).batch_size_eval == 2
    for flags, word in ((["--peft"], "--peft"), (["--int4"], "--int4"), (["--data_augmentation"], "--data_augmentation"),
                        (["--text_augmentation"], "--text_augmentation"), (["--gradient_accumulation_steps", "16"], "gradient accumulation")):
        with pytest.raises(SystemExit):
            parse_args(base + flags)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["train_dir", "valid_dir"])  # --base_model is required: nothing is downloaded
    # the collator's rule: a leading <|startoftranscript|> on every sequence is cut (shift_tokens_right puts it back)
    assert make_labels(["ab", "c"], lambda t: [101] + [ord(c) for c in t] + [100], 101) == [[97, 98, 100], [99, 100]]
    assert make_labels(["ab", "c"], lambda t: [ord(c) for c in t], 101) == [[97, 98], [99]]


def test_text_wer():
    from ssak_amd.metrics import text_wer
    r = text_wer(["a b c d", "x y"], ["a c d e", "x y"])
    assert (r["edits"], r["ref_words"]) == (2, 6) and abs(r["wer"] - 2 / 6) < 1e-15
    assert text_wer(["a b"], [""])["edits"] == 2 and text_wer([""], ["a"])["edits"] == 1
