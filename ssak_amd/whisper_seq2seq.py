"""Whisper as the reference runs it -- encoder AND text decoder (``transformers.WhisperForConditionalGeneration``;
ssak/infer/whisper_infer.py, ssak/train/transformers/whisper_train.py:432,498-507).

What it is for: transcript scoring (:meth:`WhisperSeq2Seq.score`: every token's log-probability under the audio, their sum, Whisper's
``avg_logprob`` and HF's cross-entropy; ``transcribe`` reports them per segment, data curation filters bad transcripts with them),
language identification (:meth:`WhisperSeq2Seq.detect_language`, openai-whisper's: one decoder position, a softmax over the language
tokens), generation (:meth:`WhisperSeq2Seq.generate`: greedy, beam search, sampling, each with or without timestamps;
:meth:`WhisperSeq2Seq.transcribe`, ssak_amd/whisper_transcribe.py, seeks a 30 s window through files of any length by the timestamps
it predicted and holds the temperature fallback) and full fine-tuning (ssak_amd/whisper_train.py).  Token ids are the contract: no
tokenizer is shipped; :meth:`WhisperSeq2Seq.score_text` imports ``transformers.WhisperTokenizer`` lazily.

The encoder is the HIP engine of :mod:`ssak_amd.whisper` (``arch = 1``) stopped at its hidden state, its CTC head left at zero and
never run.  The decoder is Python sequencing over C entries, the way :mod:`ssak_amd.classify` composes its head.  Weights: fp32
masters with a bf16 shadow; activations bf16, logits fp32.  Its structure:

* Two layer walks, and only these two spell a decoder layer (``ssak_gemm_bf16`` with bias / GELU epilogues for every product, q|k|v
  and the cross k|v packed; ``ssak_layernorm_fwd`` for each residual + LayerNorm).  :meth:`WhisperSeq2Seq._decoder_hidden` is the
  teacher-forced pass over [B, L] tokens (``ssak_dec_embed``, ``ssak_dec_attention_fwd``): scoring, language identification and the
  prompt of a generation, whose self-attention k|v it leaves in the cache.  Training hooks in here: with ``keep`` the same pass calls
  the entries that also write what the backward reads and keeps every buffer.  :meth:`WhisperSeq2Seq._gen_step` is one new row per
  decoder row against the cache and the cross k|v buffer, in fixed buffers (``ssak_dec_attention_step``;
  ``ssak_dec_attention_fwd`` at Lq = 1 on a cache shorter than ``STEP_SELF_MIN_KEYS``).
* One chunked vocabulary projection against the tied embedding (:meth:`WhisperSeq2Seq._project_chunks`): the logits of all ``B * L``
  rows never exist at once; the projection and what reads it (``ssak_token_logprobs``, the training loss and its backward) run over
  ``row_chunk`` rows, so the workspace is ``row_chunk * V * 4`` bytes whatever the batch.
* One generation loop (:meth:`WhisperSeq2Seq._gen_loop`: select, poll, step).  A call computes every layer's cross k|v projection of
  the encoder output once (:meth:`WhisperSeq2Seq._gen_begin`), runs the prompt (:meth:`WhisperSeq2Seq._gen_prefill`) and stays on the
  device: the host reads one pinned word every ``poll_every`` steps and the tokens once at the end.
* The selections the loop is given.  The three token-step entries (``ssak_dec_greedy_step``; ``ssak_dec_timestamp_step``: whisper's
  ``ApplyTimestampRules``; ``ssak_dec_sample_step``: a draw from the filtered distribution, ``best_of`` rows per utterance) launch one
  kernel that applies the logits processors, picks the token, and writes its log-probability, the finished flags and the next input
  row.  Beam search (:meth:`WhisperSeq2Seq._beam_step`: ``ssak_dec_beam_topk`` / ``ssak_dec_beam_select`` / ``ssak_dec_kv_reorder``)
  keeps ``beam_size`` hypotheses per utterance on the device.  The host half is numpy: :func:`rows_finalize`, :func:`beam_finalize`,
  :func:`beam_rank`.

Not built: a beam ``patience``, ``condition_on_previous_text`` / ``initial_prompt``, word timestamps, a skinny-M GEMM for the token
step, hipGraph capture of the step, an fp32-exact mode of the decoder.  LoRA adapters: ssak_amd/whisper_lora.py.  Timing: tools/bench_whisper_decoder.py,
tools/bench_whisper_generate.py, tools/bench_whisper_transcribe.py, tools/bench_whisper_beam.py, tools/bench_whisper_sample.py,
tools/bench_whisper_train.py; DESIGN.md has a section for each ("Whisper decoder", "Whisper generation", "Whisper long-form
transcription", "Whisper beam search", "Whisper sampling and temperature fallback", "Whisper fine-tuning").
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
from .whisper_lora import WhisperLoraMixin, find_adapter_config, load_adapter_folder
from .whisper_train import WhisperTrainMixin

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
    # what generate() reads (generation_config.json; eos / pad also from config.json)
    eos_token_id: Optional[int] = None
    pad_token_id: Optional[int] = None
    suppress_tokens: Optional[List[int]] = None
    begin_suppress_tokens: Optional[List[int]] = None
    task_to_id: Optional[Dict[str, int]] = None
    no_timestamps_token_id: Optional[int] = None
    # what generate(timestamps=True) reads on top: the largest index of a window's first timestamp (None: no limit) and the
    # <|nospeech|> token (None: no_timestamps_token_id - 1, where Whisper's vocabularies have it)
    max_initial_timestamp_index: Optional[int] = 50
    no_speech_token_id: Optional[int] = None
    # the regularisers of config.json: inference ignores them, forward_train() refuses any that is > 0
    dropout: float = 0.0
    attention_dropout: float = 0.0
    activation_dropout: float = 0.0
    decoder_layerdrop: float = 0.0
    encoder_layerdrop: float = 0.0

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


@dataclasses.dataclass
class GenerateResult:
    """``tokens``: per utterance the generated ids without the prompt, ending at its ``eos`` if it reached one; ``lens`` [B] their
    counts; ``token_array`` [B, n] int32, the same ids padded with ``pad`` (n = the longest); ``logprobs`` [B, n] float64, each
    token's log-softmax under the processed logits, 0 past ``lens``; ``sum_logprob`` [B]; ``avg_logprob`` = sum / (len + 1) as
    :class:`ScoreResult` has it; ``steps``: the token steps the loop ran before it stopped.  ``no_speech_prob`` [B] float64 (only
    with ``timestamps=True``, else None): the softmax probability of the no-speech token on the unprocessed logits of the
    ``<|startoftranscript|>`` row.  ``beams`` (only with ``beam_size``, else None): per utterance the ``beam_size`` candidates
    ``(tokens, sum_logprob)`` in finalisation order -- the finished sequences in the order they finished, then the live ones by
    descending sum; the other fields describe the candidate the ranking chose, ``sum_logprob`` being the device's fp32 running sum;
    ``beam_logprobs``: per utterance and candidate the per-token log-probs (float64 arrays, as long as the candidate's tokens).
    ``samples`` (only with ``temperature > 0``, else None): per utterance the ``best_of`` drawn candidates ``(tokens, sum_logprob)`` in
    row order, ``sample_logprobs`` their per-token log-probs; the other fields describe the candidate the ranking chose."""
    tokens: List[List[int]]
    lens: np.ndarray
    token_array: np.ndarray
    logprobs: np.ndarray
    sum_logprob: np.ndarray
    avg_logprob: np.ndarray
    steps: int
    no_speech_prob: Optional[np.ndarray] = None
    beams: Optional[list] = None
    beam_logprobs: Optional[list] = None
    samples: Optional[list] = None
    sample_logprobs: Optional[list] = None


# The shortest self-attention cache on which the token step runs ssak_dec_attention_step; below it, ssak_dec_attention_fwd at
# Lq = 1.  tools/bench_whisper_generate.py times the two side by side (DESIGN.md "Whisper generation"): the step kernel wins
# beyond the run-to-run range on the cross buffer and on a 448-key cache, at B = 1 and B = 32; on a 64-key cache both are at the
# launch floor (about 4 us) and their ranges overlap, so a cache of up to 64 keys keeps the older entry.
STEP_SELF_MIN_KEYS = 65


@dataclasses.dataclass
class _GenState:
    """What the stepping primitives of :meth:`WhisperSeq2Seq.generate` share.  ``step_cross`` / ``step_self_min_keys``: which
    attention entry the token step runs -- ssak_dec_attention_step on the cross buffer / on a cache of at least that many keys
    (None: never), ssak_dec_attention_fwd at Lq = 1 otherwise."""
    B: int
    S: int
    D: int
    cap: int                              # rows of the self-attention cache
    enc: torch.Tensor                     # [B, S, D] bf16
    enc_lens: Optional[torch.Tensor]      # int32 [B] on the device, validated once
    enc_lens_host: Optional[np.ndarray]   # the same values for the older attention entry (prefill, fallback)
    cross_kv: torch.Tensor                # [layers, B * S, 2 D]
    self_kv: torch.Tensor                 # [layers, B, cap, 2 D]
    ws: torch.Tensor                      # the attention step's split workspace
    h: torch.Tensor                       # the step's activation rows, [B, D] (f: [B, ffn])
    h2: torch.Tensor
    x: torch.Tensor
    q: torch.Tensor
    ctx: torch.Tensor
    y: torch.Tensor
    f: torch.Tensor
    step_cross: bool = True
    step_self_min_keys: Optional[int] = STEP_SELF_MIN_KEYS
    t: int = 0                            # cache rows in use = the next position
    group: int = 1                        # beam search: decoder rows per utterance (the cache and the step's rows count B * group)


@dataclasses.dataclass
class _BeamState:
    """The device state of a beam search over ``B`` utterances x ``nb`` hypotheses (R = B * nb rows), advanced by
    :meth:`WhisperSeq2Seq._beam_step`: what ``ssak_dec_beam_topk`` / ``ssak_dec_beam_select`` read and write (include/ssak_hip.h)."""
    B: int
    nb: int
    P: int                                # prompt length: the reorders cover the cache rows [P, t)
    eos: int
    pad: int
    sup: Optional[torch.Tensor]
    bsup: Optional[torch.Tensor]
    ts: Optional[dict]                    # ts_begin, no_timestamps_id, max_initial; None without timestamps
    tokens: torch.Tensor                  # int32 [R, n_max]
    logprobs: torch.Tensor                # fp32 [R, n_max]
    sums: torch.Tensor                    # fp32 [B, nb]: [0, -inf, ...] at the start
    src: torch.Tensor                     # int32 [R]
    ts_last: Optional[torch.Tensor]       # int32 [R]
    cand_token: torch.Tensor              # int32 [R, nb + 1]
    cand_logprob: torch.Tensor            # fp32 [R, nb + 1]
    fin_tokens: torch.Tensor              # int32 [B, nb, n_max]
    fin_logprobs: torch.Tensor
    fin_len: torch.Tensor                 # int32 [B, nb]
    fin_sum: torch.Tensor                 # fp32 [B, nb]
    n_fin: torch.Tensor                   # int32 [B]
    done: torch.Tensor                    # uint8 [B]
    n_unf: torch.Tensor                   # int32 [1]
    h_next: torch.Tensor                  # bf16 [R, D]
    i: int = 0                            # steps taken = history entries per row


@dataclasses.dataclass
class _GenPlan:
    """The arguments of :meth:`WhisperSeq2Seq.generate`, validated and normalised by :meth:`WhisperSeq2Seq._gen_plan`."""
    prompt: Optional[np.ndarray]          # int64 [B, P]; None: the default prompt with the language this call detects
    P: int                                # prompt width
    n_max: int                            # token steps at most
    eos: int
    pad: int
    sup: Optional[torch.Tensor]           # uint8 [V] device masks (:meth:`WhisperSeq2Seq._token_mask`)
    bsup: Optional[torch.Tensor]
    group: int                            # decoder rows per utterance: beam_size, or best_of, or 1
    best_of: int                          # candidates drawn per utterance; 0: not sampling
    ts: Optional[dict] = None             # timestamps: the rules' ts_begin, no_timestamps_id, max_initial
    sot_row: Optional[int] = None         # timestamps: the prompt row no_speech_prob is read at, and its token
    no_speech_id: Optional[int] = None


def beam_finalize(tokens, sums, fin_tokens, fin_len, fin_sum, n_fin, steps: int, nb: int):
    """Host half of the beam search for one utterance: the finished sequences in the order they finished, then -- while fewer than
    ``nb`` -- the live hypotheses by ``list(np.argsort(sums))[::-1]`` (no eos, no eos term in their sum), skipping ``-inf`` ->
    [(token list, sum, finished?, index)], ``index`` = the sequence's slot in the finished store or the live hypothesis' beam (where
    its per-token log-probs are).  An utterance with neither (no allowed column at the first step) gets one empty candidate."""
    out = [([int(x) for x in fin_tokens[k, :fin_len[k]]], float(fin_sum[k]), True, k) for k in range(int(n_fin))]
    for j in list(np.argsort(sums))[::-1]:
        if len(out) >= nb:
            break
        if sums[j] > -np.inf:
            out.append(([int(x) for x in tokens[j, :steps]], float(sums[j]), False, int(j)))
    return out or [([], 0.0, False, -1)]


def beam_rank(cands, length_penalty=None) -> int:
    """whisper's MaximumLikelihoodRanker over the candidates of :func:`beam_finalize`: score = sum / length with length = the
    tokens before eos (``length_penalty`` a: sum / ((5 + length) / 6) ** a); a length of 0 scores -inf; ``np.argmax`` picks."""
    scores = []
    for toks, s, fin, _ in cands:
        n = len(toks) - 1 if fin else len(toks)
        scores.append(-np.inf if n == 0 else s / (n if length_penalty is None else ((5 + n) / 6) ** length_penalty))
    return int(np.argmax(scores))


def _rank_and_pack(cands, lps, pad: int, length_penalty=None) -> dict:
    """Per utterance its candidates ``cands[b]`` ([(token list, sum, finished?, index)]) and their per-token log-probs ``lps[b]``:
    :func:`beam_rank` picks one -> the :class:`GenerateResult` fields that describe the chosen ones, padded with ``pad`` / 0."""
    picks = [beam_rank(c, length_penalty) for c in cands]
    chosen = [c[w][0] for c, w in zip(cands, picks)]
    lens = np.array([len(c) for c in chosen], dtype=np.int64)
    n = int(lens.max())
    tok, lp = np.full((len(cands), n), pad, dtype=np.int32), np.zeros((len(cands), n), dtype=np.float64)
    for b, w in enumerate(picks):
        tok[b, :lens[b]] = chosen[b]
        lp[b, :lens[b]] = lps[b][w]
    s = np.array([c[w][1] for c, w in zip(cands, picks)], dtype=np.float64)
    return dict(tokens=chosen, lens=lens, token_array=tok, logprobs=lp, sum_logprob=s, avg_logprob=s / (lens + 1))


def rows_finalize(tokens, logprobs, steps: int, eos: int, pad: int, best_of: int = 0, length_penalty=None) -> dict:
    """Host half of greedy decoding and of sampling: ``tokens`` int32 / ``logprobs`` float64 [R, >= steps] as the loop wrote them
    (a finished row goes on with ``pad`` and log-probability 0) -> the :class:`GenerateResult` fields other than ``steps`` and
    ``no_speech_prob``.  A row ends with its first ``eos`` (``pad == eos`` or not), or after ``steps`` tokens.  ``best_of`` = 0:
    greedy, one row per utterance.  ``best_of`` = n >= 1: n adjacent rows per utterance, ranked by :func:`beam_rank`, all of them
    listed in ``samples`` / ``sample_logprobs`` in row order."""
    tok, lp = tokens[:, :steps], logprobs[:, :steps]
    lens = np.array([int(np.argmax(r == eos)) + 1 if (r == eos).any() else steps for r in tok], dtype=np.int64)
    n = int(lens.max())
    # a row's sum: sampling adds up the whole row, greedy its tokens in a row as long as the longest (the orders differ by a rounding)
    sums = lp.sum(-1) if best_of else np.where(np.arange(n) < lens[:, None], lp[:, :n], 0.0).sum(-1)
    group = max(best_of, 1)
    cands, lps = [], []
    for b in range(len(tok) // group):
        rows = range(b * group, (b + 1) * group)
        cands.append([(tok[r, :lens[r]].tolist(), float(sums[r]), bool((tok[r] == eos).any()), r) for r in rows])
        lps.append([lp[r, :lens[r]].copy() for r in rows])
    out = _rank_and_pack(cands, lps, pad, length_penalty)
    if best_of:
        out.update(samples=[[(c[0], c[1]) for c in cs] for cs in cands], sample_logprobs=lps)
    return out


def sample_call_seed(seed: int) -> int:
    """The 64-bit seed ``ssak_dec_sample_step`` gets for a :meth:`WhisperSeq2Seq.generate` call with ``seed``: state 0 from
    ``np.random.SeedSequence(seed)``, then one 64-bit LCG step, as :class:`ssak_amd.model.Wav2Vec2ForCTC` derives its dropout seeds.
    Within the call the kernel's draws differ by step and row."""
    s = int(np.random.SeedSequence(int(seed)).generate_state(1, dtype=np.uint64)[0])
    return (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)


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


class WhisperSeq2Seq(WhisperTrainMixin, WhisperLoraMixin):
    """``WhisperSeq2Seq.from_pretrained(folder)``; :meth:`encode`, :meth:`decode_logprobs`, :meth:`score`, :meth:`detect_language`,
    :meth:`generate`, :meth:`transcribe`; training: :meth:`forward_train`, :meth:`backward`, :meth:`save_pretrained`
    (ssak_amd/whisper_train.py).  The module docstring names the parts."""

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
    def from_pretrained(cls, folder: str, device: str = "cuda:0", freeze_encoder: bool = False) -> "WhisperSeq2Seq":
        """An HF ``WhisperForConditionalGeneration`` folder: ``config.json``, ``model.safetensors`` / ``pytorch_model.bin``,
        ``generation_config.json`` for ``lang_to_id`` and ``decoder_start_token_id`` (else the ``<|xx|>`` entries of
        ``added_tokens.json`` / ``vocab.json``) and for what :meth:`generate` needs: ``eos_token_id``, ``pad_token_id``,
        ``suppress_tokens``, ``begin_suppress_tokens``, ``task_to_id``, ``no_timestamps_token_id``.  Unsupported configurations are
        refused by name.  A PEFT folder (an ``adapter_config.json`` in it or below it, as the reference's inference looks for one) loads
        the base model its ``base_model_name_or_path`` names, a local folder, and merges the LoRA adapter into it
        (ssak_amd/whisper_lora.py)."""
        from .checkpoint import load_state_dict_file
        if not os.path.isdir(folder):
            raise FileNotFoundError(f"{folder}: not a model folder (nothing is downloaded: pass a local folder in the HuggingFace layout)")
        adapter_dir = find_adapter_config(folder)
        if adapter_dir is not None:
            return load_adapter_folder(cls, folder, adapter_dir, device, freeze_encoder)
        with open(os.path.join(folder, "config.json")) as f:
            d = json.load(f)
        extra = {}
        gen = os.path.join(folder, "generation_config.json")
        lang_to_id = None
        if os.path.isfile(gen):
            with open(gen) as f:
                g = json.load(f)
            lang_to_id = g.get("lang_to_id")
            for key in ("decoder_start_token_id", "eos_token_id", "pad_token_id", "suppress_tokens", "begin_suppress_tokens", "task_to_id",
                        "no_timestamps_token_id", "max_initial_timestamp_index", "no_speech_token_id"):
                if g.get(key) is not None:
                    extra[key] = g[key]
            if isinstance(extra.get("eos_token_id"), list):  # (newer generation configs list several: the first is <|endoftext|>)
                extra["eos_token_id"] = extra["eos_token_id"][0]
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
        model.freeze_encoder = bool(freeze_encoder)  # (training only: forward_train / backward / WhisperAdamW leave the encoder alone)
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
    def _linear(self, x, w, bias, epilogue=hip.EPI_NONE, out=None, **kw):
        """An nn.Linear: x [M, K] against w [N, K] (+ bias, ``epilogue``) -> [M, N] bf16, fresh unless ``out`` is given."""
        M, K = x.shape
        N = w.shape[0]
        out = torch.empty((M, N), dtype=torch.bfloat16, device=self.device) if out is None else out
        return hip.gemm(x, w, out, M, N, K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=epilogue, **kw)

    def _decoder_hidden(self, enc: torch.Tensor, tokens: np.ndarray, enc_lens=None, pos_offset: int = 0, cross_kv=None, self_cache=None,
                        keep: Optional[list] = None):
        """The decoder stack on ``tokens`` [B, L] (teacher forcing) -> the final LayerNorm's output [B * L, D] bf16.  The prefill
        of :meth:`generate` passes ``cross_kv`` [layers, B * S, 2 D] (read instead of projecting the encoder output again) and
        ``self_cache`` [layers, B, cap, 2 D] (receives each layer's self-attention k|v rows).

        ``keep`` (a list, training): the same walk through the entries that also write what :meth:`backward` reads -- LayerNorm with
        mean / rstd, attention with its log-sum-exp, fc1 with its pre-activation -- every buffer fresh; ``keep`` receives one dict
        per layer (``ln1`` / ``ln2`` / ``ln3`` as (r, out, mean, rstd), ``qkv``, ``ctx_s``, ``lse_s``, ``q_c``, ``kv_c``, ``ctx_c``,
        ``lse_c``, ``pre``, ``f``) and the final LayerNorm's tuple is returned in place of its output.  Without it nothing outlives
        its layer: the residual stream alternates between two buffers and every LayerNorm writes the one ``x``."""
        cfg = self.config
        B, S, D = enc.shape
        if tokens.shape[0] != B:
            raise ValueError(f"{tokens.shape[0]} token sequences for {B} encoder outputs")
        L, nh = tokens.shape[1], cfg.decoder_attention_heads
        enc2 = enc.reshape(B * S, D)
        lora = self._lora_active()  # unmerged adapters: their products follow the base q_proj / v_proj products
        if lora and cross_kv is not None:
            raise RuntimeError("a generation's cross k|v buffer holds no adapter: generate() runs on the merged shadow (lora_merged())")
        bf = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=self.device)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            h = hip.dec_embed(self._w("embed_tokens.weight"), self._w("embed_positions.weight"), tokens, pos_offset)
            x, spare = (bf(B * L, D), [bf(B * L, D)]) if keep is None else (None, None)

            def norm(y, res, name):
                """r = res + y (``res`` itself where ``y`` is None), LayerNorm ``name`` of it -> (r, out, mean, rstd)"""
                g, b = self._f(name + ".weight"), self._f(name + ".bias")
                if keep is not None:
                    r, out, mean, rstd = res if y is None else bf(B * L, D), bf(B * L, D), f32(B * L), f32(B * L)
                    hip.layernorm_fwd_stats(y, res, g, b, out, mean, rstd, r_out=None if y is None else r)
                    return r, out, mean, rstd
                r = res
                if y is not None:
                    r, spare[0] = spare[0], res
                hip.layernorm_fwd(y, res, g, b, None if y is None else r, x)
                return r, x, None, None

            def attend(q, k, v, Lk, **mask):
                """-> (ctx, lse | None)"""
                if keep is not None:
                    return hip.dec_attention_fwd_lse(q, k, v, B, L, Lk, nh, **mask)
                return hip.dec_attention_fwd(q, k, v, B, L, Lk, nh, **mask), None

            def fc1(x, p):
                """GELU in fc1's epilogue -> (pre-activation | None, GELU of it)"""
                pre = None if keep is None else bf(B * L, cfg.decoder_ffn_dim)
                return pre, self._linear(x, self._w(p + "fc1.weight"), self._f(p + "fc1.bias"), hip.EPI_GELU, aux_out=pre)

            ln = norm(None, h, "layers.0.self_attn_layer_norm")
            for l in range(cfg.decoder_layers):
                p = f"layers.{l}."
                s = {"ln1": ln}  # (the layer's buffers live in ``s`` alone: without ``keep`` they go when the next layer starts)
                # causal self-attention: q | k | v in one product, the attention reads its three column blocks in place
                s["qkv"] = self._linear(ln[1], self._w(p + "self_attn.q_proj.weight", 3), self._f(p + "self_attn.q_proj.bias", 3))
                if lora:
                    self._lora_fwd(l, "self_attn", "q_proj", ln[1], s["qkv"][:, :D], s)
                    self._lora_fwd(l, "self_attn", "v_proj", ln[1], s["qkv"][:, 2 * D:], s)
                if self_cache is not None:
                    self_cache[l, :, :L].copy_(s["qkv"][:, D:].view(B, L, 2 * D))
                s["ctx_s"], s["lse_s"] = attend(s["qkv"][:, :D], s["qkv"][:, D:2 * D], s["qkv"][:, 2 * D:], L, causal=True)
                y = self._linear(s["ctx_s"], self._w(p + "self_attn.out_proj.weight"), self._f(p + "self_attn.out_proj.bias"))
                s["ln2"] = ln = norm(y, ln[0], p + "encoder_attn_layer_norm")
                # cross-attention: the layer's k | v projection of the encoder output, [B * S, 2 D]
                s["q_c"] = self._linear(ln[1], self._w(p + "encoder_attn.q_proj.weight"), self._f(p + "encoder_attn.q_proj.bias"))
                s["kv_c"] = cross_kv[l] if cross_kv is not None else self._linear(enc2, self._w(p + "encoder_attn.k_proj.weight", 2),
                                                                                  self._f(p + "encoder_attn.k_proj.bias", 2))
                if lora:
                    self._lora_fwd(l, "encoder_attn", "q_proj", ln[1], s["q_c"], s)
                    self._lora_fwd(l, "encoder_attn", "v_proj", enc2, s["kv_c"][:, D:], s)
                s["ctx_c"], s["lse_c"] = attend(s["q_c"], s["kv_c"][:, :D], s["kv_c"][:, D:], S, klens=enc_lens)
                y = self._linear(s["ctx_c"], self._w(p + "encoder_attn.out_proj.weight"), self._f(p + "encoder_attn.out_proj.bias"))
                s["ln3"] = ln = norm(y, ln[0], p + "final_layer_norm")
                # feed-forward
                s["pre"], s["f"] = fc1(ln[1], p)
                y = self._linear(s["f"], self._w(p + "fc2.weight"), self._f(p + "fc2.bias"))
                ln = norm(y, ln[0], f"layers.{l + 1}.self_attn_layer_norm" if l + 1 < cfg.decoder_layers else "layer_norm")
                if keep is not None:
                    keep.append(s)
        return ln[1] if keep is None else ln

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

    def _project_chunks(self, x: torch.Tensor):
        """:meth:`_project` of ``x`` [R, D], ``min(row_chunk, R)`` rows at a time (the workspace is never larger than the call needs,
        nor than ``row_chunk`` rows) -> per chunk (first row, rows, logits).  Every chunk's logits sit in the one workspace: the
        consumer enqueues its reads before it asks for the next."""
        R = x.shape[0]
        chunk = min(self.row_chunk, R)
        for r0 in range(0, R, chunk):
            n = min(chunk, R - r0)
            yield r0, n, self._project(x[r0:r0 + n], chunk)

    @staticmethod
    def _ids(ids, what: str) -> np.ndarray:
        """Token ids or labels [B, L], a tensor or host values -> a contiguous int64 host array."""
        a = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
        if a.ndim != 2 or a.shape[1] < 1:
            raise ValueError(f"{what} [B, L], got shape {a.shape}")
        return np.ascontiguousarray(a, dtype=np.int64)

    @staticmethod
    def _enc_lens(enc_lens, B: int, S: int) -> Optional[np.ndarray]:
        """The encoder frames cross-attention may see, validated once -> int32 host values [B] (None: all S)."""
        if enc_lens is None:
            return None
        lens = hip._host_i32(enc_lens, B, "enc_lens")
        if lens.min() < 1 or lens.max() > S:
            raise ValueError(f"enc_lens: {B} values in [1, {S}] expected, got {lens}")
        return lens

    @classmethod
    def _tokens(cls, tokens, lens):
        t = cls._ids(tokens, "tokens")
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
            for r0, n, logits in self._project_chunks(x):
                full[r0:r0 + n].copy_(logits)
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
        V = self.config.vocab_size
        with torch.cuda.device(self.device):
            parts = [hip.token_logprobs(logits, V, targets[r0:r0 + n])[1] for r0, n, logits in self._project_chunks(x)]
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
        return self._detect_language(self._as_enc(enc_or_audio), enc_lens)

    def _detect_language(self, enc: torch.Tensor, enc_lens=None, cross_kv=None):
        """:meth:`detect_language` on an encoder output; ``cross_kv``: the cross k|v buffer of a :meth:`generate` call, read
        instead of projecting the encoder output once more."""
        B = enc.shape[0]
        sot = np.full((B, 1), self.config.decoder_start_token_id, dtype=np.int64)
        x = self._decoder_hidden(enc, sot, enc_lens, cross_kv=cross_kv)
        with torch.cuda.device(self.device):
            parts = [hip.token_logprobs(logits, self.config.vocab_size, None, self.lang_ids)[2:] for _, _, logits in self._project_chunks(x)]
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

    # ------------------------------------------------------------------ generation
    def _gen_begin(self, enc: torch.Tensor, enc_lens=None, cap: Optional[int] = None, step_cross: bool = True,
                   step_self_min_keys: Optional[int] = STEP_SELF_MIN_KEYS, group: int = 1) -> _GenState:
        """Everything a call computes once: the twelve cross k|v projections of the encoder output into ONE [layers, B * S, 2 D]
        buffer (1.77 GB at whisper-small, B = 32), the empty self-attention cache, the encoder lengths (validated here, uploaded
        here, read by the kernels from the device ever after).  ``group`` > 1 (beam search): the cache and the step's activation rows
        count ``B * group``; the cross buffer stays at B utterances and the step reads it through ``ssak_dec_attention_step_grouped``."""
        cfg = self.config
        B, S, D = enc.shape
        group = int(group)
        if group > 1 and not step_cross:
            raise ValueError("group > 1: the beams share the cross k|v buffer through the step kernel only (step_cross)")
        R = B * group
        cap = cfg.max_target_positions if cap is None else int(cap)
        lens_host = self._enc_lens(enc_lens, B, S)
        lens_dev = None if lens_host is None else torch.from_numpy(lens_host).to(self.device)
        with torch.cuda.device(self.device):
            nl, nh = cfg.decoder_layers, cfg.decoder_attention_heads
            cross_kv = torch.empty((nl, B * S, 2 * D), dtype=torch.bfloat16, device=self.device)
            enc2 = enc.reshape(B * S, D)
            for l in range(nl):
                p = f"layers.{l}.encoder_attn.k_proj."
                hip.gemm(enc2, self._w(p + "weight", 2), cross_kv[l], B * S, 2 * D, D, lda=D, ldb=D, ldc=2 * D, bias=self._f(p + "bias", 2))
            bf = lambda n: torch.empty((R, n), dtype=torch.bfloat16, device=self.device)
            return _GenState(B=B, S=S, D=D, cap=cap, enc=enc, enc_lens=lens_dev, enc_lens_host=lens_host, cross_kv=cross_kv,
                             self_kv=torch.zeros((nl, R, cap, 2 * D), dtype=torch.bfloat16, device=self.device),
                             ws=hip.dec_attention_step_workspace(R, nh, 0, self.device), h=bf(D), h2=bf(D), x=bf(D), q=bf(D), ctx=bf(D), y=bf(D),
                             f=bf(cfg.decoder_ffn_dim), step_cross=bool(step_cross), step_self_min_keys=step_self_min_keys, group=group)

    def _gen_prefill(self, st: _GenState, prompt: np.ndarray, also_row: Optional[int] = None, also_target: Optional[int] = None):
        """One teacher-forced pass over ``prompt`` [B, P] at positions 0 .. P - 1 (``ssak_dec_attention_fwd``, causal), its
        self-attention k|v into the cache -> the logits [B, Vp] fp32 of the LAST prompt row only.  With ``also_row`` (a prompt
        position) that row is projected as well, first, through the same workspace, and the return value is (logits of the last
        row, log-softmax of column ``also_target`` on row ``also_row`` [B] fp32 on the device: ``ssak_token_logprobs``)."""
        B, P = prompt.shape
        if st.t != 0 or P > st.cap:
            raise ValueError(f"prefill of {P} tokens into a cache of {st.cap} rows with {st.t} in use")
        # (beam search: the prompt runs once per utterance, its k|v into the cache rows of beam 0, then copied once to the
        # utterance's other beams: a slot that holds no hypothesis after the first step and is filled later needs them too)
        x = self._decoder_hidden(st.enc, prompt, st.enc_lens_host, 0, cross_kv=st.cross_kv,
                                 self_cache=st.self_kv if st.group == 1 else st.self_kv[:, ::st.group])
        if st.group > 1:
            kv = st.self_kv.view(st.self_kv.shape[0], B, st.group, st.cap, 2 * st.D)
            kv[:, :, 1:, :P].copy_(kv[:, :, :1, :P].expand(-1, -1, st.group - 1, -1, -1))
        st.t = P
        row = lambda i: self._project(x.view(B, P, st.D)[:, i].contiguous(), B)
        with torch.cuda.device(self.device):
            if also_row is None:
                return row(P - 1)
            if not 0 <= also_row < P:
                raise ValueError(f"also_row {also_row} outside the prompt's {P} positions")
            lp = hip.token_logprobs(row(also_row), self.config.vocab_size, np.full(B, int(also_target), dtype=np.int32))[1]
            return row(P - 1), lp

    def _gen_attend(self, st: _GenState, kind: str, q, kv, n_keys: int):
        """ctx [B, D] of the one new row: ``kv`` [B, rows, 2 D] is a layer's cache (``kind`` "self": the first ``n_keys`` rows
        are in use) or its cross k|v ("cross": all S rows, the encoder lengths on top)."""
        D, nh = st.D, self.config.decoder_attention_heads
        if kind == "cross" and st.step_cross:  # the rows of an utterance (beams, samples) read its one cross k|v
            return hip.dec_attention_step_grouped(q, kv[:, :, :D], kv[:, :, D:], n_keys, nh, st.group, klens=st.enc_lens, workspace=st.ws,
                                                  ctx=st.ctx)
        if kind == "self" and st.step_self_min_keys is not None and n_keys >= st.step_self_min_keys:
            return hip.dec_attention_step(q, kv[:, :, :D], kv[:, :, D:], n_keys, nh, workspace=st.ws, ctx=st.ctx)
        rows = kv.shape[1]
        kv2 = kv.reshape(kv.shape[0] * rows, 2 * D)
        if kind == "self":  # the causal mask of a query at position n_keys - 1 hides the unused rows of the cache
            return hip.dec_attention_fwd(q, kv2[:, :D], kv2[:, D:], kv.shape[0], 1, rows, nh, causal=True, q_offset=n_keys - 1, ctx=st.ctx)
        return hip.dec_attention_fwd(q, kv2[:, :D], kv2[:, D:], st.B, 1, rows, nh, klens=st.enc_lens_host, ctx=st.ctx)

    def _gen_step(self, st: _GenState, h_in: torch.Tensor) -> torch.Tensor:
        """One token: ``h_in`` [B, D] bf16, the embedding row at position ``st.t`` (``ssak_dec_greedy_step``'s ``h_next``), through
        the layers against the cache and the cross buffer -> the logits [B, Vp] fp32 of that position.  Nothing is read back."""
        cfg = self.config
        B, D, t = st.B * st.group, st.D, st.t  # (B: the step's rows)
        if t >= st.cap:
            raise ValueError(f"the cache of {st.cap} rows is full")
        with torch.cuda.device(self.device):
            h, h2, x = st.h, st.h2, st.x
            h.copy_(h_in)
            hip.layernorm_fwd(None, h, self._f("layers.0.self_attn_layer_norm.weight"), self._f("layers.0.self_attn_layer_norm.bias"), None, x)
            for l in range(cfg.decoder_layers):
                p = f"layers.{l}."
                w3, b3 = self._w(p + "self_attn.q_proj.weight", 3), self._f(p + "self_attn.q_proj.bias", 3)
                self._linear(x, w3[:D], b3[:D], out=st.q)
                # the new row's k | v straight into row t of the layer's cache: C's row stride is one utterance's cache
                hip.gemm(x, w3[D:], st.self_kv[l, :, t], B, 2 * D, D, lda=D, ldb=D, ldc=st.cap * 2 * D, bias=b3[D:])
                ctx = self._gen_attend(st, "self", st.q, st.self_kv[l], t + 1)
                self._linear(ctx, self._w(p + "self_attn.out_proj.weight"), self._f(p + "self_attn.out_proj.bias"), out=st.y)
                hip.layernorm_fwd(st.y, h, self._f(p + "encoder_attn_layer_norm.weight"), self._f(p + "encoder_attn_layer_norm.bias"), h2, x)
                h, h2 = h2, h
                self._linear(x, self._w(p + "encoder_attn.q_proj.weight"), self._f(p + "encoder_attn.q_proj.bias"), out=st.q)
                ctx = self._gen_attend(st, "cross", st.q, st.cross_kv[l].view(st.B, st.S, 2 * D), st.S)
                self._linear(ctx, self._w(p + "encoder_attn.out_proj.weight"), self._f(p + "encoder_attn.out_proj.bias"), out=st.y)
                hip.layernorm_fwd(st.y, h, self._f(p + "final_layer_norm.weight"), self._f(p + "final_layer_norm.bias"), h2, x)
                h, h2 = h2, h
                self._linear(x, self._w(p + "fc1.weight"), self._f(p + "fc1.bias"), hip.EPI_GELU, out=st.f)
                self._linear(st.f, self._w(p + "fc2.weight"), self._f(p + "fc2.bias"), out=st.y)
                nxt = f"layers.{l + 1}.self_attn_layer_norm." if l + 1 < cfg.decoder_layers else "layer_norm."
                hip.layernorm_fwd(st.y, h, self._f(nxt + "weight"), self._f(nxt + "bias"), h2, x)
                h, h2 = h2, h
            st.h, st.h2 = h, h2
            st.t = t + 1
            return self._project(x, B)

    def _beam_begin(self, st: _GenState, P: int, n_max: int, eos: int, pad: int, sup, bsup, ts: Optional[dict]) -> _BeamState:
        B, nb = st.B, st.group
        R, dev = B * nb, self.device
        with torch.cuda.device(dev):
            sums = torch.full((B, nb), float("-inf"), dtype=torch.float32, device=dev)
            sums[:, 0] = 0.0
            i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)
            f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            return _BeamState(B=B, nb=nb, P=P, eos=eos, pad=pad, sup=sup, bsup=bsup, ts=ts, tokens=i32(R, n_max, fill=pad), logprobs=f32(R, n_max),
                              sums=sums, src=i32(R), ts_last=None if ts is None else i32(R, fill=-1), cand_token=i32(R, nb + 1, fill=-1),
                              cand_logprob=torch.full((R, nb + 1), float("-inf"), dtype=torch.float32, device=dev),
                              fin_tokens=i32(B, nb, n_max, fill=pad), fin_logprobs=f32(B, nb, n_max), fin_len=i32(B, nb), fin_sum=f32(B, nb),
                              n_fin=i32(B), done=torch.zeros(B, dtype=torch.uint8, device=dev), n_unf=i32(1),
                              h_next=torch.empty((R, st.D), dtype=torch.bfloat16, device=dev))

    def _beam_step(self, st: _GenState, bs: _BeamState, logits: torch.Tensor, last: bool = False):
        """One step of the beam search on ``logits`` [B * nb, Vp] (the prefill's logits repeated per beam, or :meth:`_gen_step`'s):
        ``ssak_dec_beam_topk``, ``ssak_dec_beam_select`` and ``ssak_dec_kv_reorder`` over the cache rows that can differ between
        the beams of an audio, [P, st.t): the prompt's rows [0, P) are the same in every beam since :meth:`_gen_prefill`.
        ``bs.h_next`` is then the input of the next :meth:`_gen_step` (not formed when ``last``).  Nothing is read back."""
        V, i = self.config.vocab_size, bs.i
        tsk = {} if bs.ts is None else dict(timestamps=True, tokens=bs.tokens, ts_last=bs.ts_last, **bs.ts)
        with torch.cuda.device(self.device):
            hip.dec_beam_topk(logits, V, bs.nb, done=bs.done, cand_token=bs.cand_token, cand_logprob=bs.cand_logprob, eos_id=bs.eos, t=i,
                              suppress=bs.sup, begin_suppress=bs.bsup, first=i == 0, **tsk)
            hip.dec_beam_select(bs.cand_token, bs.cand_logprob, bs.nb, V, sum_logprob=bs.sums, src=bs.src, tokens=bs.tokens, logprobs=bs.logprobs,
                                t=i, fin_tokens=bs.fin_tokens, fin_logprobs=bs.fin_logprobs, fin_len=bs.fin_len, fin_sum=bs.fin_sum, n_fin=bs.n_fin,
                                done=bs.done, n_unfinished=bs.n_unf, eos_id=bs.eos, pad_id=bs.pad, ts_last=bs.ts_last,
                                ts_begin=0 if bs.ts is None else bs.ts["ts_begin"], embed_tokens=self._w("embed_tokens.weight"),
                                embed_positions=self._w("embed_positions.weight"), next_pos=bs.P + i, h_next=None if last else bs.h_next)
            if not last and bs.nb > 1 and st.t > bs.P:
                hip.dec_kv_reorder(st.self_kv, bs.src, bs.nb, bs.P, st.t)
        bs.i = i + 1

    def _gen_loop(self, st: _GenState, logits: torch.Tensor, n_max: int, poll_every: int, select, n_unf: torch.Tensor, h_next: torch.Tensor) -> int:
        """The loop of :meth:`generate`, greedy and beam: ``select(logits, i, last)`` closes step ``i`` (the token step, or
        :meth:`_beam_step`) and leaves the next input rows in ``h_next`` unless ``last``; every ``poll_every`` steps the host reads
        ``n_unf`` through a pinned word and stops at 0; :meth:`_gen_step` gives the next logits -> the steps taken."""
        word = torch.zeros(1, dtype=torch.int32).pin_memory()
        for i in range(n_max):
            last = i + 1 == n_max
            select(logits, i, last)
            if last:
                break
            if poll_every and (i + 1) % poll_every == 0:
                word.copy_(n_unf, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                if int(word[0]) == 0:
                    break
            logits = self._gen_step(st, h_next)
        return i + 1

    def _generate_beam(self, st: _GenState, logits: torch.Tensor, pl: _GenPlan, poll_every: int, length_penalty, no_speech) -> GenerateResult:
        """The loop of :meth:`generate` with ``beam_size``: lock step over B * nb rows, the host polls ``n_unfinished`` (audios that
        do not hold nb finished sequences yet), one copy at the end, finalisation and ranking on the host."""
        B, nb = st.B, st.group
        bs = self._beam_begin(st, pl.P, pl.n_max, pl.eos, pl.pad, pl.sup, pl.bsup, pl.ts)
        with torch.cuda.device(self.device):
            steps = self._gen_loop(st, logits.repeat_interleave(nb, dim=0), pl.n_max, poll_every,
                                   lambda logits, i, last: self._beam_step(st, bs, logits, last=last), bs.n_unf, bs.h_next)
            host = lambda x: x.cpu().numpy()
            tok, lp, sums = host(bs.tokens).reshape(B, nb, -1), host(bs.logprobs).reshape(B, nb, -1), host(bs.sums)
            ftok, flp, flen, fsum, nfin = host(bs.fin_tokens), host(bs.fin_logprobs), host(bs.fin_len), host(bs.fin_sum), host(bs.n_fin)
            if no_speech is not None:
                no_speech = np.exp(no_speech.double().cpu().numpy())
        beams = [beam_finalize(tok[b], sums[b], ftok[b], flen[b], fsum[b], nfin[b], steps, nb) for b in range(B)]
        lps = [[(flp[b, k, :flen[b, k]] if fin else lp[b, k, :steps] if k >= 0 else lp[b, 0, :0]).astype(np.float64) for _, _, fin, k in cands]
               for b, cands in enumerate(beams)]
        return GenerateResult(steps=steps, no_speech_prob=no_speech, beams=[[(c[0], c[1]) for c in cands] for cands in beams], beam_logprobs=lps,
                              **_rank_and_pack(beams, lps, pl.pad, length_penalty))

    def _token_mask(self, ids, what: str) -> Optional[torch.Tensor]:
        """A list of token ids -> the uint8 [V] device mask ``ssak_dec_greedy_step`` reads (None for an empty list)."""
        V = self.config.vocab_size
        ids = np.asarray([] if ids is None else list(ids), dtype=np.int64).reshape(-1)
        if not ids.size:
            return None
        if ids.min() < 0 or ids.max() >= V:
            raise ValueError(f"{what}: ids outside [0, {V})")
        m = np.zeros(V, dtype=np.uint8)
        m[ids] = 1
        return torch.from_numpy(m).to(self.device)

    def default_prompt(self, B: int, language=None, task: str = "transcribe", timestamps: bool = False) -> np.ndarray:
        """``[<|startoftranscript|>, language, task, <|notimestamps|>]`` per utterance, [B, 4] (``language``: one code or B codes;
        a model without language tokens gets ``[<|startoftranscript|>, <|notimestamps|>]``).  ``timestamps``: the same without
        the closing ``<|notimestamps|>``, [B, 3] (or [B, 1])."""
        cfg = self.config
        if cfg.no_timestamps_token_id is None:
            raise ValueError("the model folder names no no_timestamps_token_id (generation_config.json): pass prompt=")
        tail = [] if timestamps else [cfg.no_timestamps_token_id]
        codes = cfg.lang_to_id or {}
        if not codes:
            return np.tile(np.array([[cfg.decoder_start_token_id] + tail], dtype=np.int64), (B, 1))
        if language is None:
            raise ValueError("default_prompt needs the language (one code or one per utterance); generate() detects it when none is given")
        langs = [language] * B if isinstance(language, str) else list(language)
        if len(langs) != B:
            raise ValueError(f"{len(langs)} languages for {B} utterances")
        for c in langs:
            if c not in codes:
                raise ValueError(f"language {c!r}: the model knows {sorted(codes)}")
        if not cfg.task_to_id or task not in cfg.task_to_id:
            raise ValueError(f"task {task!r}: the model folder's task_to_id is {cfg.task_to_id}")
        return np.array([[cfg.decoder_start_token_id, codes[c], cfg.task_to_id[task]] + tail for c in langs], dtype=np.int64)

    def _gen_plan(self, B: int, prompt, language, task, max_new_tokens, suppress_tokens, begin_suppress_tokens, eos_token_id, poll_every: int,
                  timestamps: bool, beam_size, length_penalty, temperature: float, best_of) -> _GenPlan:
        """The arguments of :meth:`generate` for ``B`` utterances, validated and normalised; launches nothing (the two masks are uploaded)."""
        cfg = self.config
        if not temperature >= 0.0 or temperature == float("inf"):
            raise ValueError(f"temperature {temperature}: a finite value >= 0 is expected")
        n_samp = 0
        if temperature > 0.0:
            if beam_size is not None:
                raise ValueError("beam_size with temperature > 0: whisper samples there instead of searching; pass best_of")
            n_samp = 1 if best_of is None else int(best_of)
            if not 1 <= n_samp <= 8:
                raise ValueError(f"best_of {best_of}: 1 to 8 candidates per utterance are built")
        if beam_size is not None:
            beam_size = int(beam_size)
            if not 1 <= beam_size <= 8:
                raise ValueError(f"beam_size {beam_size}: 1 to 8 hypotheses per utterance are built")
        elif length_penalty is not None and not n_samp:
            raise ValueError("length_penalty ranks the candidates of a beam search or of best_of samples: pass beam_size, or temperature and best_of")
        if timestamps and cfg.no_timestamps_token_id is None:
            raise ValueError("timestamps=True: the model folder names no no_timestamps_token_id (generation_config.json), the timestamp ids are "
                             "those above it")
        if beam_size is not None and B * beam_size > 65535:
            raise ValueError(f"{B} utterances x beam_size {beam_size} = {B * beam_size} decoder rows: at most 65535 in one call")
        if B * n_samp > 65535:
            raise ValueError(f"{B} utterances x best_of {n_samp} = {B * n_samp} decoder rows: at most 65535 in one call")
        V, maxp = cfg.vocab_size, cfg.max_target_positions
        eos = cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
        if eos is None:
            raise ValueError("no eos_token_id: the model folder names none, pass eos_token_id=")
        pad = eos if cfg.pad_token_id is None else int(cfg.pad_token_id)
        # the default prompt is [<|startoftranscript|>, language, task, <|notimestamps|>]: where the language is to be detected only its
        # width is known yet
        if prompt is None and language is None and bool(cfg.lang_to_id):
            if not cfg.task_to_id or task not in cfg.task_to_id or cfg.no_timestamps_token_id is None:
                raise ValueError(f"task {task!r} / no_timestamps_token_id: the model folder's generation_config.json names neither: pass prompt=")
            P = 3 if timestamps else 4
        else:
            if prompt is None:
                prompt = self.default_prompt(B, language, task, timestamps)
            prompt = np.asarray(prompt.cpu() if torch.is_tensor(prompt) else prompt, dtype=np.int64)
            prompt = np.ascontiguousarray(np.broadcast_to(prompt, (B, prompt.shape[-1])) if prompt.ndim == 1 else prompt)
            if prompt.ndim != 2 or prompt.shape[0] != B or prompt.shape[1] < 1:
                raise ValueError(f"prompt [B, P] or [P] for {B} utterances, got shape {prompt.shape}")
            P = prompt.shape[1]
        n_max = (min(maxp // 2, maxp - P) if timestamps else maxp - P) if max_new_tokens is None else int(max_new_tokens)
        if n_max < 1 or P + n_max > maxp:
            raise ValueError(f"prompt of {P} + max_new_tokens {n_max} tokens: the decoder has max_target_positions = {maxp} positions")
        if poll_every < 0:
            raise ValueError("poll_every must be >= 0")
        pl = _GenPlan(prompt=prompt, P=P, n_max=n_max, eos=eos, pad=pad, best_of=n_samp, group=max(n_samp, 1) if beam_size is None else beam_size,
                      sup=self._token_mask(cfg.suppress_tokens if suppress_tokens is None else suppress_tokens, "suppress_tokens"),
                      bsup=self._token_mask(cfg.begin_suppress_tokens if begin_suppress_tokens is None else begin_suppress_tokens,
                                            "begin_suppress_tokens"))
        if timestamps:
            sot = cfg.decoder_start_token_id  # (the default prompt starts with it)
            sot_rows = [0] if prompt is None else [int(np.argmax(r == sot)) if (r == sot).any() else -1 for r in prompt]
            if min(sot_rows) < 0 or len(set(sot_rows)) != 1:
                raise ValueError("timestamps=True: no_speech_prob is read at the prompt's <|startoftranscript|>, which must sit at one position "
                                 "in every row")
            pl.sot_row = sot_rows[0]
            pl.no_speech_id = int(cfg.no_timestamps_token_id) - 1 if cfg.no_speech_token_id is None else int(cfg.no_speech_token_id)
            if not 0 <= pl.no_speech_id < V:
                raise ValueError(f"no_speech_token_id {pl.no_speech_id} outside [0, {V})")
            pl.ts = dict(ts_begin=int(cfg.no_timestamps_token_id) + 1, no_timestamps_id=int(cfg.no_timestamps_token_id),
                         max_initial=-1 if cfg.max_initial_timestamp_index is None else int(cfg.max_initial_timestamp_index))
        return pl

    def generate(self, enc_or_audio, prompt=None, language=None, task: str = "transcribe", max_new_tokens: Optional[int] = None, enc_lens=None,
                 suppress_tokens=None, begin_suppress_tokens=None, eos_token_id: Optional[int] = None, poll_every: int = 8,
                 timestamps: bool = False, beam_size: Optional[int] = None, length_penalty: Optional[float] = None, temperature: float = 0.0,
                 best_of: Optional[int] = None, seed: int = 1234) -> GenerateResult:
        """Greedy transcription (temperature 0), beam search with ``beam_size``, or sampling with ``temperature > 0``, of a batch in lock
        step -> :class:`GenerateResult`.

        ``prompt`` [B, P] or [P] ids (one P for the batch); by default ``[<|startoftranscript|>, language, task,
        <|notimestamps|>]``, where ``language = None`` runs :meth:`detect_language`'s pass first (on this call's cross k|v buffer) and gives each
        utterance its own token.
        ``max_new_tokens``: by default what fits, ``max_target_positions - P``; more is a ``ValueError``.  ``suppress_tokens`` /
        ``begin_suppress_tokens`` / ``eos_token_id`` override the model folder's ``generation_config.json``.  ``enc_lens`` [B]:
        the encoder frames cross-attention may see.

        Memory: every layer's cross k|v projection of the encoder output is computed ONCE per call into a [layers, B * S, 2 D]
        bf16 buffer -- 1.77 GB at whisper-small with B = 32 -- next to the [layers, B, P + max_new_tokens, 2 D] cache.
        The host reads nothing per token: every ``poll_every`` steps it reads the count of unfinished utterances through a pinned
        word and stops at 0 (``poll_every = 0``: never, the loop runs ``max_new_tokens`` steps); tokens and log-probabilities
        are copied once at the end.

        ``timestamps=True``: whisper's timestamp rules (``ssak_dec_timestamp_step``; the first timestamp at most
        ``max_initial_timestamp_index``), the default prompt without ``<|notimestamps|>``, by default at most
        ``min(max_target_positions // 2, max_target_positions - P)`` tokens (whisper's ``sample_len``), and ``no_speech_prob``
        in the result.  The default leaves the call as it was.

        ``beam_size`` in [1, 8]: whisper's ``BeamSearchDecoder`` (DESIGN.md "Whisper beam search": no patience) with ``MaximumLikelihoodRanker(length_penalty)``.  The prompt, the language pass and ``no_speech_prob`` run once
        per utterance; the token step runs ``B * beam_size`` rows whose cross-attention shares the utterance's one cross k|v buffer;
        the self-attention cache follows the hypotheses (``ssak_dec_kv_reorder``).  ``GenerateResult.beams`` lists every candidate.
        ``beam_size=None`` is the greedy path, unchanged.

        ``temperature > 0``: every token is drawn from ``softmax(x / temperature)`` over the filtered row (``ssak_dec_sample_step``,
        DESIGN.md "Whisper sampling and temperature fallback"), with and without ``timestamps``.  ``best_of`` in [1, 8] (None: 1)
        draws that many candidates per utterance -- the prompt runs once per utterance, the rows of an utterance share its cross k|v
        buffer as beams do and differ by their row index in the draw -- and ``MaximumLikelihoodRanker(length_penalty)`` picks one;
        ``GenerateResult.samples`` lists them all.  The same ``seed`` gives the same result.  ``beam_size`` together with
        ``temperature > 0`` is refused (whisper drops the beam there; :func:`ssak_amd.whisper_transcribe.transcribe` does the
        dropping).  ``temperature = 0`` (the default) leaves the call as it was and ignores ``best_of`` and ``seed``."""
        if self._lora_active():  # the token step and the cross k|v buffer read the shadow: merge the adapters for the call
            with self.lora_merged():
                return self.generate(enc_or_audio, prompt=prompt, language=language, task=task, max_new_tokens=max_new_tokens, enc_lens=enc_lens,
                                     suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, eos_token_id=eos_token_id,
                                     poll_every=poll_every, timestamps=timestamps, beam_size=beam_size, length_penalty=length_penalty,
                                     temperature=temperature, best_of=best_of, seed=seed)
        enc = self._as_enc(enc_or_audio)
        B, V = enc.shape[0], self.config.vocab_size
        pl = self._gen_plan(B, prompt, language, task, max_new_tokens, suppress_tokens, begin_suppress_tokens, eos_token_id, poll_every,
                            bool(timestamps), beam_size, length_penalty, float(temperature), best_of)
        st = self._gen_begin(enc, enc_lens, cap=pl.P + pl.n_max, group=pl.group)
        prompt = pl.prompt
        if prompt is None:  # (the language pass reads this call's cross k|v buffer)
            prompt = self.default_prompt(B, self._detect_language(enc, st.enc_lens_host, cross_kv=st.cross_kv)[0], task, timestamps)
        no_speech = None
        if pl.ts is None:
            logits = self._gen_prefill(st, prompt)
        else:
            logits, no_speech = self._gen_prefill(st, prompt, also_row=pl.sot_row, also_target=pl.no_speech_id)
        if beam_size is not None:
            return self._generate_beam(st, logits, pl, poll_every, length_penalty, no_speech)
        E, Pz = self._w("embed_tokens.weight"), self._w("embed_positions.weight")
        R = B * st.group  # the step's rows: one per utterance, best_of per utterance when sampling
        with torch.cuda.device(self.device):
            tokens = torch.full((R, pl.n_max), pl.pad, dtype=torch.int32, device=self.device)
            logprobs = torch.zeros((R, pl.n_max), dtype=torch.float32, device=self.device)
            finished = torch.zeros(R, dtype=torch.uint8, device=self.device)
            n_unf = torch.zeros(1, dtype=torch.int32, device=self.device)
            h_next = torch.empty((R, st.D), dtype=torch.bfloat16, device=self.device)
            step, rules = hip.dec_greedy_step, {}
            if pl.ts is not None:
                step = hip.dec_timestamp_step
                rules = dict(pl.ts, ts_last=torch.full((R,), -1, dtype=torch.int32, device=self.device))
            if pl.best_of:
                step = hip.dec_sample_step
                rules.update(temperature=temperature, seed=sample_call_seed(seed))
                if pl.best_of > 1:
                    logits = logits.repeat_interleave(pl.best_of, dim=0)
            select = lambda logits, i, last: step(logits, V, finished=finished, n_unfinished=n_unf, tokens=tokens, logprobs=logprobs, t=i,
                                                  eos_id=pl.eos, pad_id=pl.pad, suppress=pl.sup, begin_suppress=pl.bsup, first=i == 0,
                                                  embed_tokens=E, embed_positions=Pz, next_pos=pl.P + i, h_next=None if last else h_next, **rules)
            steps = self._gen_loop(st, logits, pl.n_max, poll_every, select, n_unf, h_next)
            tok = tokens[:, :steps].cpu().numpy()
            lp = logprobs[:, :steps].double().cpu().numpy()
            if no_speech is not None:
                no_speech = np.exp(no_speech.double().cpu().numpy())
        return GenerateResult(steps=steps, no_speech_prob=no_speech, **rows_finalize(tok, lp, steps, pl.eos, pl.pad, pl.best_of, length_penalty))

    def transcribe(self, waveforms, language=None, task: str = "transcribe", no_speech_threshold: Optional[float] = 0.6,
                   logprob_threshold: Optional[float] = -1.0, batch_size: int = 8, **kw):
        """Long-form transcription with timestamps: :func:`ssak_amd.whisper_transcribe.transcribe`."""
        from .whisper_transcribe import transcribe
        return transcribe(self, waveforms, language=language, task=task, no_speech_threshold=no_speech_threshold,
                          logprob_threshold=logprob_threshold, batch_size=batch_size, **kw)
