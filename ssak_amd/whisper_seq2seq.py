"""Whisper as the reference runs it -- encoder AND text decoder (``transformers.WhisperForConditionalGeneration``;
ssak/infer/whisper_infer.py, ssak/train/transformers/whisper_train.py:432,498-507) -- as a teacher-forced pass, with the two uses
that need no generation loop:

* transcript scoring: the log-probability of every token of a GIVEN token sequence under the audio, their sum, Whisper's
  ``avg_logprob`` (whisper/decoding.py: ``sum / (len + 1)``) and HF's seq2seq cross-entropy (the mean over labels other than
  -100) -- what ``transcribe`` reports per segment and the forward half of the fine-tuning loss; data curation filters bad
  transcripts with it;
* language identification: openai-whisper's ``detect_language`` -- one decoder position after ``<|startoftranscript|>``, a
  softmax restricted to the language tokens.

The encoder is the HIP engine of :mod:`ssak_amd.whisper` (``arch = 1``) stopped at its hidden state, its CTC head left at zero
and never run.  The decoder is Python sequencing over C entries, the way :mod:`ssak_amd.classify` composes its head:
``ssak_dec_embed``, ``ssak_dec_attention_fwd`` (causal self-attention into the packed q|k|v buffer, cross-attention into the
encoder-side k|v buffer), ``ssak_token_logprobs`` (ssak_amd/csrc/whisper_decoder.hip), ``ssak_gemm_bf16`` with its bias / GELU
epilogues for every projection including the vocabulary projection against the tied embedding, and ``ssak_layernorm_fwd`` for
the residual + LayerNorm between them.  Weights: fp32 masters with a bf16 shadow; activations bf16, logits fp32.  The logits of
all ``B * L`` rows are never materialised at once: the vocabulary projection and the log-softmax run over chunks of
``ROW_CHUNK`` rows, so the workspace is ``ROW_CHUNK * V * 4`` bytes whatever the batch.

Token ids are the contract (no tokenizer is needed, and none is shipped); :meth:`WhisperSeq2Seq.score_text` is a convenience
that imports ``transformers.WhisperTokenizer`` lazily.  Not built: KV cache, generation, timestamps, fallback temperatures, beam
search, training / LoRA, an fp32-exact mode of the decoder.  Timing: tools/bench_whisper_decoder.py (DESIGN.md "Whisper decoder").
"""
from __future__ import annotations

import dataclasses
import json
import os
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hip
from .whisper import WhisperCTCConfig, WhisperEncoderForCTC

ROW_CHUNK = 256  # rows of the vocabulary projection in flight (51 865 columns: 53 MB of fp32 logits)
N_SAMPLES = 480000  # Whisper's 30 s window at 16 kHz
_LANG_TOKEN = re.compile(r"^<\|([a-z]{2,3})\|>$")


@dataclasses.dataclass
class WhisperSeq2SeqConfig:
    """What ``config.json`` / ``generation_config.json`` of a ``WhisperForConditionalGeneration`` folder say (whisper-small by default)."""
    vocab_size: int = 51865
    num_mel_bins: int = 80
    d_model: int = 768
    encoder_layers: int = 12
    encoder_attention_heads: int = 12
    encoder_ffn_dim: int = 3072
    decoder_layers: int = 12
    decoder_attention_heads: int = 12
    decoder_ffn_dim: int = 3072
    max_source_positions: int = 1500
    max_target_positions: int = 448
    decoder_start_token_id: int = 50258
    scale_embedding: bool = False
    tie_word_embeddings: bool = True
    activation_function: str = "gelu"
    lang_to_id: Optional[Dict[str, int]] = None  # language code ("fr") -> token id

    def __post_init__(self):
        for what, heads in (("encoder", self.encoder_attention_heads), ("decoder", self.decoder_attention_heads)):
            if self.d_model % heads or self.d_model // heads != hip.DEC_HEAD_DIM:
                raise ValueError(f"{what} head dimension {self.d_model / heads:g} (d_model {self.d_model} / {heads} heads): the supported "
                                 f"head dimension is {hip.DEC_HEAD_DIM}")
        if self.scale_embedding:
            raise ValueError("scale_embedding = true: the scaled token embedding is not built")
        if not self.tie_word_embeddings:
            raise ValueError("tie_word_embeddings = false: an untied proj_out is not built (the vocabulary projection reads embed_tokens)")
        if self.activation_function != "gelu":
            raise ValueError(f"activation_function {self.activation_function!r}: only gelu is built")
        if self.d_model > 1536:
            raise ValueError(f"d_model {self.d_model}: the LayerNorm row kernel takes up to 1536 columns")

    @classmethod
    def from_hf_dict(cls, d: dict, **extra) -> "WhisperSeq2SeqConfig":
        names = {f.name for f in dataclasses.fields(cls)}
        return cls(**{k: v for k, v in dict(d, **extra).items() if k in names and v is not None})


@dataclasses.dataclass
class ScoreResult:
    """Per utterance (numpy float64 [B]): ``sum_logprob``; ``avg_logprob`` = sum / (n_scored + 1); ``loss`` = -sum / n_scored, the
    utterance's mean cross-entropy.  ``batch_loss``: HF's ``.loss`` of the batch, the mean over all its labels other than -100.
    ``logprobs`` [B, L - 1] as :meth:`WhisperSeq2Seq.decode_logprobs` returns them, on the host."""
    sum_logprob: np.ndarray
    avg_logprob: np.ndarray
    loss: np.ndarray
    batch_loss: float
    n_scored: np.ndarray
    logprobs: np.ndarray


def _decoder_layout(cfg: WhisperSeq2SeqConfig):
    """name -> (offset, numel, shape) in the flat parameter buffer, every tensor on a 16-byte boundary of the bf16 shadow.  q, k, v
    of an attention are adjacent, weights and biases, so that the packed [3 D, D] (self) and [2 D, D] (cross k|v) operands are
    slices; Whisper's k_proj has no bias: its slot is synthetic, stays zero and is not part of a checkpoint."""
    D, F, Vp = cfg.d_model, cfg.decoder_ffn_dim, (cfg.vocab_size + 7) // 8 * 8
    shapes = [("embed_tokens.weight", (Vp, D)), ("embed_positions.weight", (cfg.max_target_positions, D))]
    for l in range(cfg.decoder_layers):
        p = f"layers.{l}."
        for attn in ("self_attn", "encoder_attn"):
            shapes += [(p + f"{attn}.{proj}.weight", (D, D)) for proj in ("q_proj", "k_proj", "v_proj", "out_proj")]
            shapes += [(p + f"{attn}.{proj}.bias", (D,)) for proj in ("q_proj", "k_proj", "v_proj", "out_proj")]
            shapes += [(p + f"{attn}_layer_norm.weight", (D,)), (p + f"{attn}_layer_norm.bias", (D,))]
        shapes += [(p + "fc1.weight", (F, D)), (p + "fc1.bias", (F,)), (p + "fc2.weight", (D, F)), (p + "fc2.bias", (D,)),
                   (p + "final_layer_norm.weight", (D,)), (p + "final_layer_norm.bias", (D,))]
    shapes += [("layer_norm.weight", (D,)), ("layer_norm.bias", (D,))]
    layout, off = {}, 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        layout["model.decoder." + name] = (off, n, shape)
        off += (n + 7) // 8 * 8
    return layout, off


class WhisperSeq2Seq:
    """``WhisperSeq2Seq.from_pretrained(folder)``; :meth:`encode`, :meth:`decode_logprobs`, :meth:`score`, :meth:`detect_language`."""

    def __init__(self, config: WhisperSeq2SeqConfig, device: str = "cuda:0", seed: int = 69):
        if not torch.cuda.is_available():
            raise RuntimeError("ssak_amd needs an MI355X: there is no CPU fallback for the acoustic model")
        self.config = config
        self.device = torch.device(device)
        self.name_or_path: Optional[str] = None
        self.row_chunk = ROW_CHUNK
        # the encoder: driven only through forward_hidden; its CTC head (8 inert classes) stays at zero and is never run
        self.encoder = WhisperEncoderForCTC(WhisperCTCConfig(
            vocab_size=8, num_mel_bins=config.num_mel_bins, d_model=config.d_model, encoder_layers=config.encoder_layers,
            encoder_attention_heads=config.encoder_attention_heads, encoder_ffn_dim=config.encoder_ffn_dim,
            max_source_positions=config.max_source_positions), device=device, seed=seed).eval()
        self.layout, total = _decoder_layout(config)
        with torch.cuda.device(self.device):
            self.dec_params = torch.zeros(total, dtype=torch.float32, device=self.device)
            self.dec_shadow = torch.zeros(total, dtype=torch.bfloat16, device=self.device)
        self._logits_ws = None
        codes = config.lang_to_id or {}
        self.lang_codes: List[str] = sorted(codes, key=codes.get)  # in token-id order, as whisper's tokenizer lists them
        self.lang_ids = np.array([codes[c] for c in self.lang_codes], dtype=np.int32)

    # ------------------------------------------------------------------ parameters
    def dec_param(self, name: str) -> torch.Tensor:
        off, n, shape = self.layout[name]
        return self.dec_params[off:off + n].view(shape)

    def _w(self, name: str, rows: int = 1) -> torch.Tensor:
        """bf16 shadow of a weight; ``rows`` > 1 takes that many adjacent tensors as one matrix (q|k|v, k|v)."""
        off, n, shape = self.layout["model.decoder." + name]
        return self.dec_shadow[off:off + rows * n].view(rows * shape[0], *shape[1:])

    def _f(self, name: str, rows: int = 1) -> torch.Tensor:
        """fp32 master of a bias / LayerNorm vector (``rows`` adjacent ones as one vector)."""
        off, n, _ = self.layout["model.decoder." + name]
        return self.dec_params[off:off + rows * n]

    def sync_decoder_shadow(self):
        with torch.cuda.device(self.device):
            hip.check(hip.lib.ssak_cast_f32_bf16(hip.ptr(self.dec_params), hip.ptr(self.dec_shadow), self.dec_params.numel(), hip.stream()))

    def load_decoder_state_dict(self, sd: Dict[str, torch.Tensor]):
        """``model.decoder.*`` tensors of a transformers state dict; every decoder parameter must be there (k_proj has no bias)."""
        V = self.config.vocab_size
        for name, (off, n, shape) in self.layout.items():
            if name.endswith("k_proj.bias"):
                continue
            if name not in sd:
                raise ValueError(f"the checkpoint has no {name} (not a WhisperForConditionalGeneration model)")
            t = torch.as_tensor(sd[name]).to(torch.float32)
            want = (V,) + tuple(shape[1:]) if name.endswith("embed_tokens.weight") else tuple(shape)
            if tuple(t.shape) != want:
                raise RuntimeError(f"size mismatch for {name}: {tuple(t.shape)} vs {want}")
            self.dec_params[off:off + t.numel()].copy_(t.reshape(-1).to(self.device))  # (the vocabulary's padding rows stay zero)
        self.sync_decoder_shadow()
        return self

    @classmethod
    def from_pretrained(cls, folder: str, device: str = "cuda:0") -> "WhisperSeq2Seq":
        """An HF ``WhisperForConditionalGeneration`` folder: ``config.json``, ``model.safetensors`` / ``pytorch_model.bin``,
        ``generation_config.json`` for ``lang_to_id`` and ``decoder_start_token_id`` (else the ``<|xx|>`` entries of
        ``added_tokens.json`` / ``vocab.json``).  Unsupported configurations are refused by name."""
        from .checkpoint import load_state_dict_file
        if not os.path.isdir(folder):
            raise FileNotFoundError(f"{folder}: not a model folder (nothing is downloaded: pass a local folder in the HuggingFace layout)")
        with open(os.path.join(folder, "config.json")) as f:
            d = json.load(f)
        extra = {}
        gen = os.path.join(folder, "generation_config.json")
        lang_to_id = None
        if os.path.isfile(gen):
            with open(gen) as f:
                g = json.load(f)
            lang_to_id = g.get("lang_to_id")
            if g.get("decoder_start_token_id") is not None:
                extra["decoder_start_token_id"] = g["decoder_start_token_id"]
        if not lang_to_id:
            lang_to_id = {}
            for name in ("added_tokens.json", "vocab.json"):
                path = os.path.join(folder, name)
                if os.path.isfile(path):
                    with open(path) as f:
                        lang_to_id.update({k: v for k, v in json.load(f).items() if _LANG_TOKEN.match(k)})
        extra["lang_to_id"] = {_LANG_TOKEN.match(k).group(1) if _LANG_TOKEN.match(k) else k: int(v) for k, v in lang_to_id.items()}
        cfg = WhisperSeq2SeqConfig.from_hf_dict(d, **extra)
        sd = load_state_dict_file(folder)
        emb = sd.get("model.decoder.embed_tokens.weight")
        if "proj_out.weight" in sd and emb is not None and not torch.equal(sd["proj_out.weight"], emb):
            raise ValueError("proj_out.weight differs from model.decoder.embed_tokens.weight: an untied proj_out is not built")
        model = cls(cfg, device=device)
        enc = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.encoder.")}
        absent = [n for n in model.encoder.layout if n not in enc and not n.startswith("ctc_head.") and not n.endswith("k_proj.bias")]
        if absent:
            raise ValueError(f"{folder}: the checkpoint has no model.{absent[0]}")
        model.encoder.load_state_dict({k: v for k, v in enc.items() if k in model.encoder.layout}, strict=False)
        model.load_decoder_state_dict(sd)
        model.name_or_path = folder
        return model

    # ------------------------------------------------------------------ encoder
    def features(self, waveforms: torch.Tensor, lens=None) -> torch.Tensor:
        """[B, T] fp32 16 kHz waveforms -> Whisper input features [B, mels, 3000]: ``pad_or_trim`` to the 30 s window and the
        log-mel spectrogram, on the device (``ssak_logmel_whisper``)."""
        w = torch.as_tensor(waveforms, dtype=torch.float32).to(self.device).contiguous()
        with torch.cuda.device(self.device):
            return hip.logmel_whisper(w, None if lens is None else torch.as_tensor(lens), n_samples=N_SAMPLES)

    def encode(self, input_features: torch.Tensor) -> torch.Tensor:
        """input_features [B, mels, 2 S] fp32 -> the encoder's last hidden state [B, S, D] bf16."""
        hidden, _ = self.encoder.forward_hidden(torch.as_tensor(input_features, dtype=torch.float32))
        return hidden

    def _as_enc(self, x) -> torch.Tensor:
        """An encoder output [B, S, D] bf16 as it is; input features [B, mels, frames] fp32 through the encoder; waveforms [B, T]
        fp32 (16 kHz) through the log-mel front end and the encoder."""
        x = torch.as_tensor(x)
        if x.dim() == 3 and x.dtype == torch.bfloat16:
            if x.shape[2] != self.config.d_model:
                raise ValueError(f"encoder output of width {x.shape[2]}, d_model is {self.config.d_model}")
            return x.to(self.device).contiguous()
        if x.dim() == 3:
            return self.encode(x)
        if x.dim() == 2:
            return self.encode(self.features(x))
        raise ValueError(f"expected an encoder output [B, S, D] (bf16), input features [B, mels, frames] or waveforms [B, T]; got {tuple(x.shape)}")

    # ------------------------------------------------------------------ decoder
    def _linear(self, x, w, bias, epilogue=hip.EPI_NONE):
        M, K = x.shape
        N = w.shape[0]
        out = torch.empty((M, N), dtype=torch.bfloat16, device=self.device)
        return hip.gemm(x, w, out, M, N, K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=epilogue)

    def _decoder_hidden(self, enc: torch.Tensor, tokens: np.ndarray, enc_lens=None, pos_offset: int = 0) -> torch.Tensor:
        """The decoder stack on ``tokens`` [B, L] (teacher forcing) -> the final LayerNorm's output [B * L, D] bf16."""
        cfg = self.config
        B, S, D = enc.shape
        if tokens.shape[0] != B:
            raise ValueError(f"{tokens.shape[0]} token sequences for {B} encoder outputs")
        L, nh = tokens.shape[1], cfg.decoder_attention_heads
        enc2 = enc.reshape(B * S, D)
        with torch.cuda.device(self.device):
            h = hip.dec_embed(self._w("embed_tokens.weight"), self._w("embed_positions.weight"), tokens, pos_offset)
            h2, x = torch.empty_like(h), torch.empty_like(h)
            hip.layernorm_fwd(None, h, self._f("layers.0.self_attn_layer_norm.weight"), self._f("layers.0.self_attn_layer_norm.bias"), None, x)
            for l in range(cfg.decoder_layers):
                p = f"layers.{l}."
                # causal self-attention: q | k | v in one product, the attention reads its three column blocks in place
                qkv = self._linear(x, self._w(p + "self_attn.q_proj.weight", 3), self._f(p + "self_attn.q_proj.bias", 3))
                ctx = hip.dec_attention_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, L, L, nh, causal=True, q_offset=0)
                y = self._linear(ctx, self._w(p + "self_attn.out_proj.weight"), self._f(p + "self_attn.out_proj.bias"))
                hip.layernorm_fwd(y, h, self._f(p + "encoder_attn_layer_norm.weight"), self._f(p + "encoder_attn_layer_norm.bias"), h2, x)
                h, h2 = h2, h
                # cross-attention: the layer's k | v projection of the encoder output, [B * S, 2 D]
                q = self._linear(x, self._w(p + "encoder_attn.q_proj.weight"), self._f(p + "encoder_attn.q_proj.bias"))
                kv = self._linear(enc2, self._w(p + "encoder_attn.k_proj.weight", 2), self._f(p + "encoder_attn.k_proj.bias", 2))
                ctx = hip.dec_attention_fwd(q, kv[:, :D], kv[:, D:], B, L, S, nh, klens=enc_lens)
                y = self._linear(ctx, self._w(p + "encoder_attn.out_proj.weight"), self._f(p + "encoder_attn.out_proj.bias"))
                hip.layernorm_fwd(y, h, self._f(p + "final_layer_norm.weight"), self._f(p + "final_layer_norm.bias"), h2, x)
                h, h2 = h2, h
                # feed-forward, GELU in fc1's epilogue
                f = self._linear(x, self._w(p + "fc1.weight"), self._f(p + "fc1.bias"), hip.EPI_GELU)
                y = self._linear(f, self._w(p + "fc2.weight"), self._f(p + "fc2.bias"))
                nxt = f"layers.{l + 1}.self_attn_layer_norm." if l + 1 < cfg.decoder_layers else "layer_norm."
                hip.layernorm_fwd(y, h, self._f(nxt + "weight"), self._f(nxt + "bias"), h2, x)
                h, h2 = h2, h
        return x

    def _project(self, x: torch.Tensor, n_rows: int) -> torch.Tensor:
        """Vocabulary projection of ``x`` [n, D] (n <= ``n_rows``, the chunk size the workspace is kept for) against the tied
        embedding -> fp32 logits [n, Vp] in the bounded workspace."""
        Vp, D = self._w("embed_tokens.weight").shape
        if self._logits_ws is None or self._logits_ws.shape[0] < n_rows:
            self._logits_ws = None
            self._logits_ws = torch.empty((n_rows, Vp), dtype=torch.float32, device=self.device)
        n = x.shape[0]
        logits = self._logits_ws[:n]
        hip.gemm(x, self._w("embed_tokens.weight"), logits, n, Vp, D, lda=D, ldb=D, ldc=Vp)
        return logits

    @staticmethod
    def _tokens(tokens, lens):
        t = tokens.detach().cpu().numpy() if torch.is_tensor(tokens) else np.asarray(tokens)
        if t.ndim != 2 or t.shape[1] < 1:
            raise ValueError(f"tokens [B, L], got shape {t.shape}")
        t = np.ascontiguousarray(t, dtype=np.int64)
        B, L = t.shape
        lens = np.full(B, L, dtype=np.int64) if lens is None else np.asarray(lens.cpu() if torch.is_tensor(lens) else lens, dtype=np.int64)
        if lens.shape != (B,) or lens.min() < 1 or lens.max() > L:
            raise ValueError(f"lens: {B} values in [1, {L}] expected, got {lens}")
        return t, lens

    def decode_logits(self, enc, tokens, enc_lens=None) -> torch.Tensor:
        """The logits of EVERY position, [B, L, V] fp32, in one piece: for tests and small shapes (``32 x 448 x 51 865`` is 3 GB;
        the scoring paths never hold more than ``row_chunk`` rows)."""
        enc = self._as_enc(enc)
        t, _ = self._tokens(tokens, None)
        x = self._decoder_hidden(enc, t, enc_lens)
        with torch.cuda.device(self.device):
            full = torch.empty((x.shape[0], self._w("embed_tokens.weight").shape[0]), dtype=torch.float32, device=self.device)
            chunk = min(self.row_chunk, x.shape[0])
            for r0 in range(0, x.shape[0], chunk):
                n = min(chunk, x.shape[0] - r0)
                full[r0:r0 + n].copy_(self._project(x[r0:r0 + n], chunk))
        return full.view(t.shape[0], t.shape[1], -1)[:, :, :self.config.vocab_size]

    def decode_logprobs(self, enc, tokens, lens=None, enc_lens=None) -> torch.Tensor:
        """log p(``tokens[:, i + 1]`` | ``tokens[:, :i + 1]``, audio) -> [B, L - 1] fp32 on the device; positions past ``lens`` are 0.
        ``enc``: as :meth:`_as_enc` takes it.  ``enc_lens`` [B]: the encoder frames cross-attention may see (None: all)."""
        enc = self._as_enc(enc)
        t, lens = self._tokens(tokens, lens)
        B, L = t.shape
        x = self._decoder_hidden(enc, t, enc_lens)
        targets = np.full((B, L), -100, dtype=np.int32)  # HF's ignore index: the row's log-probability is written as 0
        for b in range(B):
            targets[b, :lens[b] - 1] = t[b, 1:lens[b]]
        targets = targets.reshape(-1)
        V, R = self.config.vocab_size, B * L
        parts = []
        with torch.cuda.device(self.device):
            chunk = min(self.row_chunk, R)  # (the workspace is never larger than the call needs, nor than ROW_CHUNK rows)
            for r0 in range(0, R, chunk):
                n = min(chunk, R - r0)
                logits = self._project(x[r0:r0 + n], chunk)
                parts.append(hip.token_logprobs(logits, V, targets[r0:r0 + n])[1])
            lp = parts[0] if len(parts) == 1 else torch.cat(parts)
        return lp.view(B, L)[:, :L - 1]

    def score(self, enc_or_audio, tokens, lens=None, enc_lens=None) -> ScoreResult:
        """The three scores of each transcript under its audio (:class:`ScoreResult`).  ``tokens`` [B, L] start with the decoder's
        prompt (``<|startoftranscript|>`` ...); every token after the first is scored, ``lens[b] - 1`` of them."""
        t, lens = self._tokens(tokens, lens)
        lp = self.decode_logprobs(enc_or_audio, t, lens, enc_lens).double().cpu().numpy()
        n = lens - 1
        s = lp.sum(-1)
        return ScoreResult(sum_logprob=s, avg_logprob=s / (n + 1), loss=-s / np.maximum(n, 1), batch_loss=float(-s.sum() / max(int(n.sum()), 1)),
                           n_scored=n, logprobs=lp)

    def detect_language(self, enc_or_audio, enc_lens=None):
        """openai-whisper's ``detect_language``: one decoder position (``[<|startoftranscript|>]``), every non-language token
        masked, softmax, arg-max -> (codes [B], probs [B, n_lang] on the device, columns in the order of ``self.lang_codes``)."""
        if not len(self.lang_ids):
            raise ValueError("the model folder lists no language tokens (generation_config.json lang_to_id, or <|xx|> entries of "
                             "added_tokens.json / vocab.json): an English-only model has no language to detect")
        enc = self._as_enc(enc_or_audio)
        B = enc.shape[0]
        sot = np.full((B, 1), self.config.decoder_start_token_id, dtype=np.int64)
        x = self._decoder_hidden(enc, sot, enc_lens)
        with torch.cuda.device(self.device):
            parts = []
            chunk = min(self.row_chunk, B)
            for r0 in range(0, B, chunk):
                n = min(chunk, B - r0)
                logits = self._project(x[r0:r0 + n], chunk)
                parts.append(hip.token_logprobs(logits, self.config.vocab_size, None, self.lang_ids)[2:])
            argmax = torch.cat([p[0] for p in parts])
            probs = torch.cat([p[1] for p in parts])
        by_id = {int(i): c for i, c in zip(self.lang_ids, self.lang_codes)}
        return [by_id[int(i)] for i in argmax.cpu().tolist()], probs

    def score_text(self, enc_or_audio, texts: Sequence[str], language: Optional[str] = None, task: str = "transcribe") -> ScoreResult:
        """:meth:`score` of plain-text transcripts, tokenised by ``transformers.WhisperTokenizer`` read from the model folder
        (``<|startoftranscript|>`` [language, task] ``<|notimestamps|>`` text ``<|endoftext|>``).  The library itself ships no
        tokenizer: where ``transformers`` is not installed, tokenise elsewhere and call :meth:`score` with the ids."""
        try:
            from transformers import WhisperTokenizer
        except ImportError as err:
            raise ImportError("score_text() tokenises with transformers.WhisperTokenizer, which is not installed here; pass token ids to "
                              "score() instead") from err
        if self.name_or_path is None:
            raise ValueError("score_text() reads the tokenizer from the folder from_pretrained() loaded")
        tok = WhisperTokenizer.from_pretrained(self.name_or_path, language=language, task=task)
        ids = [tok(t).input_ids for t in texts]
        L = max(len(i) for i in ids)
        pad = np.full((len(ids), L), tok.eos_token_id, dtype=np.int64)
        for b, i in enumerate(ids):
            pad[b, :len(i)] = i
        return self.score(enc_or_audio, pad, [len(i) for i in ids])
