"""Long-form Whisper transcription with timestamps, as ssak/infer/whisper_infer.py asks of ``model.transcribe``: greedy decoding or
beam search under the timestamp rules, a 30 s window that seeks through the file by the timestamps it predicted, silent windows
skipped by ``no_speech_prob``, and whisper's temperature fallback -- a window whose text compresses too well or whose ``avg_logprob``
is too low is decoded again by sampling at the next temperature (``condition_on_previous_text = False``).

Files run in lock step, each with its own seek (in 10 ms frames).  One round takes, for every file that is not finished, the window
``audio[seek * 160 : seek * 160 + 480000]`` -- zero-padded, gathered on the device with torch indexing -- and runs
``features`` -> ``encode`` -> ``generate(timestamps=True)`` over that batch; the host then advances each file's seek by
:func:`segments_from_window` (whisper's own rules, a pure host function) and finished files drop out of the next round.  The
language is detected on a file's first window only.  With several temperatures :func:`decode_with_fallback` decodes a round's
windows at the first one and only the failing windows again, as one smaller batch on the same encoder output, at the next.

Deviations from openai-whisper, stated rather than fixed (DESIGN.md "Whisper long-form transcription"): the log-mel spectrogram is
taken per window (whisper takes one of the whole file, so the clamp maximum and the frames at window edges differ); the fallback
runs in lock step over a round's windows (DESIGN.md "Whisper sampling and temperature fallback").  Not built:
``condition_on_previous_text`` / ``initial_prompt``, word timestamps.
"""
from __future__ import annotations

import dataclasses
import zlib
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

HOP = 160            # samples per 10 ms frame
N_FRAMES = 3000      # frames of the 30 s window
N_SAMPLES = N_FRAMES * HOP


class Segment(NamedTuple):
    """``start`` / ``end`` in seconds from the file's beginning; ``tokens``: the slice's ids, timestamps included; ``seek``: the
    window's first frame; ``avg_logprob`` / ``no_speech_prob``: the window's."""
    start: float
    end: float
    tokens: List[int]
    seek: int
    avg_logprob: float
    no_speech_prob: float


@dataclasses.dataclass
class Window:
    """One decoded window of a file: its first frame, its frames, the sampled tokens before the eos, whisper's ``avg_logprob``
    (the sum including the eos step over tokens before eos + 1) and ``no_speech_prob``; ``temperature``: the one whose result
    stands; ``compression_ratio`` of that result's text (0 where no ``text_of`` was given)."""
    seek: int
    segment_frames: int
    tokens: List[int]
    avg_logprob: float
    no_speech_prob: float
    temperature: float = 0.0
    compression_ratio: float = 0.0


@dataclasses.dataclass
class TranscribeResult:
    """``language``: the code the file was decoded with (None for a model without language tokens); ``segments``; ``windows``:
    every window decoded, skipped ones included; ``seeks``: each window's seek and the final one, ``content_frames``."""
    language: Optional[str]
    segments: List[Segment]
    windows: List[Window]
    seeks: List[int]
    content_frames: int


def segments_from_window(tokens: Sequence[int], seek: int, segment_frames: int, ts_begin: int, eos: int, input_stride: int = 2,
                         avg_logprob: float = 0.0, no_speech_prob: float = 0.0, no_speech_threshold: Optional[float] = None,
                         logprob_threshold: Optional[float] = None):
    """whisper's ``transcribe`` for one decoded window -> (segments, new_seek).  ``tokens``: the window's sampled ids before the
    eos; ``seek`` / ``segment_frames``: the window's first frame and its frames (3000, fewer at the file's end);
    ``input_stride`` = 3000 // max_source_positions frames per timestamp step.  With ``no_speech_threshold`` the window is skipped
    (no segments, the seek moves past it) when ``no_speech_prob`` exceeds it, unless ``avg_logprob > logprob_threshold``."""
    tokens = [int(t) for t in tokens]
    time_precision = input_stride * 0.01
    offset = seek * 0.01
    if no_speech_threshold is not None and no_speech_prob > no_speech_threshold:
        if not (logprob_threshold is not None and avg_logprob > logprob_threshold):
            return [], seek + segment_frames
    ts = [t >= ts_begin for t in tokens]
    single_ending = ts[-2:] == [False, True]
    consecutive = [i + 1 for i in range(len(tokens) - 1) if ts[i] and ts[i + 1]]
    found = []
    if consecutive:
        slices = consecutive + ([len(tokens)] if single_ending else [])
        last = 0
        for cur in slices:
            sl = tokens[last:cur]
            found.append((offset + (sl[0] - ts_begin) * time_precision, offset + (sl[-1] - ts_begin) * time_precision, sl))
            last = cur
        new_seek = seek + segment_frames if single_ending else seek + (tokens[last - 1] - ts_begin) * input_stride
    else:
        duration = segment_frames * 0.01
        stamps = [t for t in tokens if t >= ts_begin]
        if stamps and stamps[-1] != ts_begin:
            duration = (stamps[-1] - ts_begin) * time_precision
        found.append((offset, offset + duration, tokens))
        new_seek = seek + segment_frames
    segments = [Segment(a, b, sl, seek, float(avg_logprob), float(no_speech_prob)) for a, b, sl in found
                if a != b and any(t < eos for t in sl)]
    return segments, new_seek


def compression_ratio(text: str) -> float:
    """whisper's ``compression_ratio``: the UTF-8 bytes of ``text`` over their zlib-compressed length."""
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def decode_with_fallback(decode_at, temperatures: Sequence[float], n: int, compression_ratio_threshold: Optional[float] = 2.4,
                         logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6, text_of=None,
                         ts_begin: Optional[int] = None):
    """whisper's ``decode_with_fallback`` over the ``n`` windows of a round, in lock step and without a model.
    ``decode_at(indices, temperature)`` decodes the given windows (indices into the round) and returns ``(tokens before eos,
    avg_logprob, no_speech_prob)`` each.  All windows are decoded at ``temperatures[0]``; a result needs a retry when its
    compression ratio exceeds ``compression_ratio_threshold`` or its ``avg_logprob`` is below ``logprob_threshold`` -- unless
    ``no_speech_prob > no_speech_threshold`` and ``avg_logprob < logprob_threshold``, which is silence and stands; the windows that
    need one are decoded again, as one smaller batch, at the next temperature; the last temperature's result stands whatever it
    is.  Any threshold may be None.  The compression ratio is taken of ``text_of(ids below ts_begin)`` (``ts_begin`` None: all
    ids); ``text_of=None`` switches that check off (the ratio is reported as 0).
    -> per window ``(tokens, avg_logprob, no_speech_prob, temperature, compression_ratio)``."""
    temperatures = [float(t) for t in temperatures]
    if not temperatures:
        raise ValueError("decode_with_fallback: at least one temperature is needed")
    out = [None] * n
    todo = list(range(n))
    for k, temp in enumerate(temperatures):
        if not todo:
            break
        decoded = decode_at(todo, temp)
        if len(decoded) != len(todo):
            raise ValueError(f"decode_at returned {len(decoded)} results for {len(todo)} windows")
        again = []
        for i, (tokens, avg_lp, ns) in zip(todo, decoded):
            ratio = 0.0
            if text_of is not None:
                ratio = compression_ratio(text_of([int(t) for t in tokens if ts_begin is None or t < ts_begin]))
            out[i] = (tokens, avg_lp, ns, temp, ratio)
            retry = text_of is not None and compression_ratio_threshold is not None and ratio > compression_ratio_threshold
            retry = retry or (logprob_threshold is not None and avg_lp < logprob_threshold)
            if no_speech_threshold is not None and ns > no_speech_threshold and logprob_threshold is not None and avg_lp < logprob_threshold:
                retry = False  # silence
            if retry and k + 1 < len(temperatures):
                again.append(i)
        todo = again
    return out


def seek_loop(content_frames: Sequence[int], decode_round, ts_begin: int, eos: int, input_stride: int = 2,
              no_speech_threshold: Optional[float] = 0.6, logprob_threshold: Optional[float] = -1.0, max_rounds: Optional[int] = None):
    """The lock-step loop over files, without a model.  ``decode_round(active, seeks, frames)`` decodes one window per active file
    (file indices, their seeks, their windows' frames) and returns per file ``(tokens before eos, avg_logprob, no_speech_prob)``,
    optionally followed by the ``temperature`` and ``compression_ratio`` of :func:`decode_with_fallback`, which the window records.
    -> per file (segments, windows, seeks).  More than ``max_rounds`` rounds is a ``RuntimeError``."""
    n = len(content_frames)
    seeks = [0] * n
    out = [([], [], [0]) for _ in range(n)]
    rounds = 0
    while True:
        active = [f for f in range(n) if seeks[f] < content_frames[f]]
        if not active:
            return out
        if max_rounds is not None and rounds >= max_rounds:
            raise RuntimeError(f"transcribe: files {active} are not finished after {max_rounds} rounds")
        rounds += 1
        frames = [min(N_FRAMES, content_frames[f] - seeks[f]) for f in active]
        decoded = decode_round(active, [seeks[f] for f in active], frames)
        for f, fr, (tokens, avg_lp, ns, *extra) in zip(active, frames, decoded):
            segs, new_seek = segments_from_window(tokens, seeks[f], fr, ts_begin, eos, input_stride, avg_lp, ns, no_speech_threshold,
                                                  logprob_threshold)
            if new_seek <= seeks[f]:
                raise RuntimeError(f"transcribe: file {f}'s seek did not advance from {seeks[f]} (tokens {list(tokens)})")
            out[f][0].extend(segs)
            out[f][1].append(Window(seeks[f], fr, [int(t) for t in tokens], float(avg_lp), float(ns), *(float(e) for e in extra)))
            seeks[f] = min(new_seek, content_frames[f])  # (whisper lets the last seek overshoot; the loop ends either way)
            out[f][2].append(seeks[f])


def transcribe(model, waveforms, language=None, task: str = "transcribe", no_speech_threshold: Optional[float] = 0.6,
               logprob_threshold: Optional[float] = -1.0, batch_size: int = 8, beam_size: Optional[int] = None, temperature=0.0,
               best_of: Optional[int] = None, compression_ratio_threshold: Optional[float] = 2.4, text_of=None, seed: int = 1234,
               _max_rounds: Optional[int] = None) -> List[TranscribeResult]:
    """``waveforms``: a list of 1-D 16 kHz waveforms of any length -> one :class:`TranscribeResult` per file.  ``language``: one code,
    one per file, or None (detected on each file's first window).  ``batch_size`` files run in lock step at a time.  ``beam_size``: every window is decoded by
    ``generate(timestamps=True, beam_size=...)`` (None: greedy).

    ``temperature``: one value or the sequence whisper's fallback tries in order (:func:`decode_with_fallback`, on
    ``compression_ratio_threshold``, ``logprob_threshold`` and ``no_speech_threshold``).  Temperature 0 decodes with ``beam_size``,
    a temperature above 0 samples with ``best_of`` candidates (``generate(temperature=..., best_of=...)``), as whisper drops the one
    or the other; a retry reads the round's encoder output again, the encoder does not run twice.  ``text_of(ids) -> str`` gives
    the text whose compression ratio is tested (None: that check is off).  ``seed``: the k-th sampling call of a transcription
    draws with ``seed + k``; the same seed gives the same result.  With a single temperature nothing is decoded twice."""
    import torch
    cfg = model.config
    temperatures = [float(temperature)] if np.isscalar(temperature) else [float(t) for t in temperature]
    if not temperatures or any(not t >= 0.0 for t in temperatures):
        raise ValueError(f"temperature {temperature}: one value >= 0 or a sequence of them")
    if cfg.no_timestamps_token_id is None or cfg.eos_token_id is None:
        raise ValueError("transcribe: the model folder names no no_timestamps_token_id / eos_token_id (generation_config.json)")
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if N_FRAMES % cfg.max_source_positions:
        raise ValueError(f"max_source_positions {cfg.max_source_positions} does not divide the window's {N_FRAMES} frames")
    waves = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waveforms]
    nf = len(waves)
    has_lang = bool(cfg.lang_to_id)
    if has_lang and language is not None:
        langs = [language] * nf if isinstance(language, str) else list(language)
        if len(langs) != nf:
            raise ValueError(f"{len(langs)} languages for {nf} files")
    else:
        langs = [None] * nf
    ts_begin, eos = int(cfg.no_timestamps_token_id) + 1, int(cfg.eos_token_id)
    stride = N_FRAMES // cfg.max_source_positions
    results: List[TranscribeResult] = []
    n_sampled = 0  # sampling calls so far: each draws with its own seed
    for g0 in range(0, nf, batch_size):
        group = list(range(g0, min(g0 + batch_size, nf)))
        content = [int(waves[f].numel()) // HOP for f in group]
        # the group's audio in one zero-padded device buffer: every window is a gather, the padding past a file's end included
        width = max(int(waves[f].numel()) for f in group) + N_SAMPLES
        audio = torch.zeros((len(group), width), dtype=torch.float32, device=model.device)
        for i, f in enumerate(group):
            audio[i, :waves[f].numel()].copy_(waves[f])
        ar = torch.arange(N_SAMPLES, device=model.device)

        def decode_round(active, seeks, frames):
            rows = torch.as_tensor(active, device=model.device)
            start = torch.as_tensor(seeks, device=model.device) * HOP
            enc = model.encode(model.features(audio[rows[:, None], start[:, None] + ar[None]]))
            if has_lang:
                todo = [i for i, a in enumerate(active) if langs[group[a]] is None]
                if todo:
                    for i, code in zip(todo, model.detect_language(enc[todo])[0]):
                        langs[group[active[i]]] = code

            def decode_at(indices, temp):
                nonlocal n_sampled
                how = dict(beam_size=beam_size)
                if temp > 0.0:
                    how = dict(temperature=temp, best_of=best_of, seed=seed + n_sampled)
                    n_sampled += 1
                whole = len(indices) == len(active)
                r = model.generate(enc if whole else enc[indices], language=[langs[group[active[i]]] for i in indices] if has_lang else None,
                                   task=task, timestamps=True, **how)
                out = []
                for b in range(len(indices)):
                    toks = r.tokens[b]
                    body = toks[:-1] if toks and toks[-1] == eos else toks
                    out.append((body, float(r.sum_logprob[b]) / (len(body) + 1), float(r.no_speech_prob[b])))
                return out

            return decode_with_fallback(decode_at, temperatures, len(active), compression_ratio_threshold, logprob_threshold,
                                        no_speech_threshold, text_of, ts_begin)

        per_file = seek_loop(content, decode_round, ts_begin, eos, stride, no_speech_threshold, logprob_threshold, _max_rounds)
        for f, cf, (segs, windows, seeks) in zip(group, content, per_file):
            results.append(TranscribeResult(language=langs[f], segments=segs, windows=windows, seeks=seeks, content_frames=cf))
    return results
