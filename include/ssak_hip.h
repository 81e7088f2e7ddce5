/* ssak_hip.h -- C ABI of libssak_hip.so: the MI355X (gfx950) acoustic-model hot path for SSAK.
 *
 * linto-ai/ssak has no FFI or plugin interface of its own: its hot path is three lines of Python
 * glue around third-party objects.  The entry points below are what a binding for
 * that path would call; each one names the reference call site it stands behind.  All pointers are
 * DEVICE pointers unless marked "host"; every entry point is asynchronous on `stream`
 * (a hipStream_t passed as void*), takes caller-owned buffers, keeps no global state and returns
 * SSAK_OK or a negative status (ssak_last_error() gives the message).  No torch types anywhere.
 *
 * Dtypes: bf16 = 16-bit brain float (uint16_t storage), activations row-major [rows, channels].
 */
#ifndef SSAK_HIP_H
#define SSAK_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAK_OK 0
#define SSAK_ERR_INVALID (-1) /* bad argument (shape, alignment, null pointer, workspace too small) */
#define SSAK_ERR_LAUNCH (-2)  /* HIP runtime / kernel launch failure */
#define SSAK_ERR_STATE (-3)   /* engine used out of order (e.g. backward before forward) */

#define SSAK_REDUCTION_SUM 0
#define SSAK_REDUCTION_MEAN 1

int ssak_version(void);
const char* ssak_last_error(void); /* host string, valid until the next failing call on this thread */

/* ---- a1: waveform normalisation -------------------------------------------------------------
 * Replaces Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm + right zero padding, reached from
 * ssak/utils/dataset.py:632 (training) and ssak/infer/transformers_infer.py:216 (inference).
 * in  [B, T] fp32 raw samples (anything beyond lens[b] is ignored), lens [B] int32 (NULL = all T)
 * out [B, T] fp32: (x - mean) / sqrt(var + 1e-7) over the first lens[b] samples, 0 beyond;
 * mask [B, T] int32 attention mask (1 valid / 0 pad) or NULL.  workspace >= ssak_wave_normalize_workspace_bytes. */
size_t ssak_wave_normalize_workspace_bytes(int B, int T);
int ssak_wave_normalize(const float* in, const int32_t* lens, int B, int T, float* out, int32_t* mask,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- a13: Whisper log-mel features ---------------------------------------------------------
 * Replaces WhisperFeatureExtractor (transformers feature_extraction_whisper.py:95-168), reached from
 * ssak/utils/dataset.py:632-637 with a Whisper processor (ssak/train/transformers/whisper_train.py:356-367).
 * wav [B, T] fp32 (lens [B] valid samples or NULL), padded / trimmed to n_samples (480000 = 30 s) -> mel
 * [B, 80, n_samples/160] fp32 (or NULL).  mel_cl_bf16 (or NULL): the same values as bf16 channels-last
 * [B, cl_rows, 80] written from row cl_lead (what the Whisper encoder's first conv reads; pad rows untouched).
 * tables: ssak_logmel_table_floats() floats, 16-byte aligned, filled once by ssak_logmel_init_tables (the FFT's twiddles, the
 * periodic Hann window and the Slaney mel filters, computed in double on the host). */
size_t ssak_logmel_table_floats(void);
int ssak_logmel_init_tables(float* tables /*device*/);
size_t ssak_logmel_workspace_bytes(int B, int n_samples);
int ssak_logmel_whisper(const float* wav, const int32_t* lens, int B, int T, int n_samples, const float* tables, float* mel,
                        void* mel_cl_bf16, int cl_rows, int cl_lead, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a9: CTC loss + gradient ----------------------------------------------------------------
 * Replaces log_softmax(fp32) -> F.ctc_loss(blank=pad_token_id, reduction, zero_infinity) and its
 * autograd backward, reached from Wav2Vec2ForCTC.forward (transformers modeling_wav2vec2.py:1705-1728)
 * under ssak/train/transformers/wav2vec_train.py:319,325,415.
 * logits [B, F, V] fp32 (raw, pre-softmax); in_lens [B] int32 valid frames; labels [B, Lmax] int32,
 * negative = padding (-100, wav2vec_train.py:100; target length = count(label >= 0)).
 * loss [1] fp32; nll [B] fp32 per-utterance negative log-likelihood (after zero_infinity) or NULL;
 * dlogits [B, F, V] fp32 = grad_scale * d loss / d logits (0 for frames >= in_lens[b]) or NULL.
 * "mean" = mean over batch of nll_b / max(target_len_b, 1).  Infeasible alignments give nll = +inf,
 * zeroed (loss and gradient) iff zero_infinity. */
size_t ssak_ctc_workspace_bytes(int B, int F, int V, int Lmax);
int ssak_ctc_loss_fwd_bwd(const float* logits, const int32_t* in_lens, const int32_t* labels, int B, int F, int V,
                          int Lmax, int blank, int reduction, int zero_infinity, float grad_scale, float* loss,
                          float* nll, float* dlogits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a12: greedy CTC decode -----------------------------------------------------------------
 * Replaces torch.argmax(logits, -1) + the collapse step of processor.batch_decode
 * (ssak/infer/transformers_infer.py:84-85): argmax over V, merge repeats, drop blank.
 * ids [B, F] int32 receives the collapsed ids left-aligned, out_lens [B] their counts. */
int ssak_ctc_greedy_decode(const float* logits, const int32_t* in_lens, int B, int F, int V, int blank, int32_t* ids,
                           int32_t* out_lens, void* stream);

/* ---- f2: audio ingest (PCM decode, mono mix, sample-rate conversion) ---------------------------
 * Replaces load_audio / conform_audio of ssak/utils/audio.py:24-154 for PCM input, reached from the Kaldi-folder loader
 * (ssak/utils/dataset.py:27-424,630-645): the segment cut is a byte range chosen by the caller (offset = int(start*sr),
 * audio.py:85-92), channels are averaged (librosa.to_mono, :118) and the rate change is torchaudio.transforms.Resample
 * with its defaults (:134): Hann-windowed sinc interpolation, lowpass_filter_width 6, rolloff 0.99.
 * ssak_pcm_to_mono_f32: raw = interleaved little-endian PCM bytes of all utterances (device), byte_offsets [B] int64 /
 *   nframes [B] int32 (device), sample_width in bytes (1 unsigned, 2 / 4 signed) -> out [B, Tmax] fp32, zero padded.
 * ssak_resample_plan / _table (host): reduced rates, filter half-width and taps; table [new_r][taps] fp32 computed in
 *   double like torchaudio's kernel.  ssak_resample_sinc: in [B, Tin] (in_lens [B] or NULL) -> out [B, Tout] with
 *   out_lens[b] = ceil(new_r * len / orig_r) valid samples (0 beyond); table on the device. */
/* ssak_read_ranges (host): n byte ranges (path, file offset, length) read with pread by `threads` native threads (a process-wide pool that outlives the call) into dst[i] (the
 *   caller's slices of a pinned staging buffer).  SSAK_ERR_INVALID with the path in ssak_last_error() for a file that cannot be
 *   opened or ends inside its range. */
int ssak_read_ranges(const char* const* paths, const int64_t* file_offsets, const int64_t* nbytes, void* const* dst, int n,
                     int threads);
/* ssak_drop_file_cache (host, measurement aid): fdatasync + posix_fadvise(DONTNEED) on each file, so that the next read comes from the
 *   storage device (bench.py's cold-cache ingest figure); returns the number of files it could not open / advise. */
int ssak_drop_file_cache(const char* const* paths, int n);
int ssak_pcm_to_mono_f32(const void* raw, const int64_t* byte_offsets, const int32_t* nframes, int B, int channels, int sample_width,
                         int Tmax, float* out, void* stream);
int ssak_resample_plan(int orig_sr, int new_sr, int* orig_r, int* new_r, int* width, int* taps);
int ssak_resample_table(int orig_sr, int new_sr, float* table /*host*/);
int ssak_resample_sinc(const float* in, const int32_t* in_lens, int B, int Tin, int orig_sr, int new_sr, const float* table /*device*/,
                       float* out, int Tout, int32_t* out_lens, void* stream);

/* ---- f3: word error counts for the evaluation step ---------------------------------------------
 * Replaces compute_metrics of ssak/train/transformers/wav2vec_train.py:110-125 after the argmax (ssak_ctc_greedy_decode):
 * batch_decode of predictions and (ungrouped) labels, remove_special_words(glue_apostrophe=False), the "wer" metric.
 * hyp_ids [B, F] / hyp_lens [B] as ssak_ctc_greedy_decode writes them; labels [B, Lmax] int32, negative = padding;
 * token_class [V] uint8: 0 letter, 1 word separator ("|"), 2 removed from the text (pad and the other "<...>" tokens),
 * 3 letter that also ends its word (the apostrophe).  edits [B] = substitutions + deletions + insertions between the
 * word sequences, ref_words [B] = reference words; WER = sum(edits) / sum(ref_words). */
size_t ssak_ctc_wer_workspace_bytes(int B, int F, int Lmax);
int ssak_ctc_wer(const int32_t* hyp_ids, const int32_t* hyp_lens, const int32_t* labels, const uint8_t* token_class, int B, int F,
                 int Lmax, int V, int32_t* edits, int32_t* ref_words, void* workspace, size_t workspace_bytes, void* stream);

/* ---- f4: CTC beam search with an ARPA n-gram LM ------------------------------------------------
 * Replaces the --arpa path of ssak/infer/transformers_infer.py:97-133 (pyctcdecode + KenLM, transformers_decoder_with_lm
 * :272-295) under a contract of its own, modelled on pyctcdecode's defaults; pyctcdecode parity unpinned.  The contract
 * (scores, merges, tie rule, LM terms) is written out in ssak_amd/lm.py.  The LM tables are built by that module from an
 * ARPA text file: a unigram trie over LABEL ids as an open-addressing hash (node, label) -> child (root = node 0),
 * unigram (log10 p, log10 backoff) pairs by word id, and one open-addressing hash per order >= 2 keyed by the full word-id
 * tuple.  Hashes: lm_hash of ssak_amd/lm.py (FNV-1a over the int32 ids + a finaliser), linear probing, every probe loop
 * bounded by the table size.  All pointers in the descriptors are device pointers. */
#define SSAK_LM_MAX_ORDER 6
#define SSAK_LM_MAX_BEAM 256
#define SSAK_LM_MAX_LABELS 1024
typedef struct {
  int order;                  /* 1..SSAK_LM_MAX_ORDER */
  int n_words;                /* word ids 0..n_words-1 */
  int bos, eos, unk;          /* word ids of <s>, </s>, <unk> */
  int trie_cap;               /* power of two */
  int n_nodes;                /* trie nodes (node_word entries) */
  const int32_t* trie;        /* [trie_cap][3] (node, label, child); node -1 = empty slot */
  const int32_t* node_word;   /* [n_nodes] word id spelled by the path to the node, or -1 */
  const float* uni;           /* [n_words][2] (log10 p, log10 backoff) */
  const int32_t* ng_keys[SSAK_LM_MAX_ORDER]; /* [k-1] for order k >= 2: [ng_cap[k-1]][k] word ids; first id -1 = empty */
  const float* ng_val[SSAK_LM_MAX_ORDER];    /* [k-1]: [ng_cap[k-1]][2] (log10 p, log10 backoff) */
  int ng_cap[SSAK_LM_MAX_ORDER];             /* powers of two */
} ssak_ngram_lm;

typedef struct {
  int beam_width;             /* 1..SSAK_LM_MAX_BEAM */
  int n_labels;               /* columns of the logits that are labels (len(tokenizer)): 1..min(V, SSAK_LM_MAX_LABELS) */
  int blank;                  /* CTC blank (pad) id, < n_labels */
  const uint8_t* label_class; /* device [n_labels]: 0 character, 1 word delimiter, 2 label without text */
  float alpha, beta;          /* LM weight, word insertion bonus */
  float beam_prune_logp;      /* candidates below best + this are dropped (-INFINITY: off) */
  float token_min_logp;       /* tokens below this log-probability are not tried (the frame's argmax always is) */
  float unk_score_offset;     /* log10 penalty of an OOV word / prefix */
} ssak_lm_beam_params;

/* logits [B, F, V] fp32 raw; in_lens [B] valid frames (NULL = F).  ids [B, F] int32: the winner's label ids left-aligned,
 * -1 beyond; n [B] their counts (-1: the utterance's prefix store overflowed, which the workspace size rules out);
 * score [B] fp32: the winner's total.  One workgroup per utterance; bit-reproducible, and an utterance's result does not
 * depend on the rest of the batch.  workspace >= ssak_ctc_lm_beam_workspace_bytes(B, F, V, beam_width). */
size_t ssak_ctc_lm_beam_workspace_bytes(int B, int F, int V, int beam_width);
int ssak_ctc_lm_beam_decode(const float* logits, const int32_t* in_lens, int B, int F, int V, const ssak_ngram_lm* lm /*host*/,
                            const ssak_lm_beam_params* params /*host*/, int32_t* ids, int32_t* n, float* score,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Batched n-gram lookup (tests compare the device tables with the host's): log10p[q] = log10 P(words[q] | ctx) with ARPA
 * backoff, ctx = ctx_ids[q][0 .. order-2] (most recent last; only the trailing run of ids >= 0 is used); NaN when an id is
 * out of range. */
int ssak_lm_query(const ssak_ngram_lm* lm /*host*/, const int32_t* ctx_ids, const int32_t* words, int Q, float* log10p,
                  void* stream);

/* ---- f1: CTC forced alignment (Viterbi trellis + backtrack) ----------------------------------
 * Replaces get_trellis + backtrack of ssak/utils/align_transcriptions.py:27-70,79-123 (USE_MAX, USE_CHAR_REPEATED),
 * reached from compute_alignment (:294-402) under tools/align_audio_transcript.py:121,335.
 * emission [F, V] fp32 log-probabilities (compute_log_probas, ssak/infer/general.py:99-101); tokens [L] int32 in [0, V);
 * col0 [F+1] = trellis column 0 supplied by the caller (the first_as_garbage variant, :38) or NULL for the running sum of
 * the blank log-probability (:40).  Outputs: trellis [F+1, L+1] fp32, bit-identical to the reference's; the path as
 * arrays indexed by time frame -- path_token[t] = token index, path_logp[t] = log of Point.score -- valid for
 * t in [path_info[1], path_info[1] + path_info[0]); path_info[0] = -1 when the walk ends without reaching token 0
 * (the reference raises RuntimeError("Failed to align ...")), -2 when a token id lies outside [0, V).
 * workspace >= ssak_ctc_align_workspace_bytes (one byte per trellis cell + one per frame).  One utterance per call, L <= 16384. */
size_t ssak_ctc_align_workspace_bytes(int F, int L);
int ssak_ctc_forced_align(const float* emission, const int32_t* tokens, int F, int V, int L, int blank, const float* col0,
                          float* trellis, int32_t* path_token, float* path_logp, int32_t* path_info /*[2]*/, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The same for B utterances in ONE launch (one workgroup each): what tools/align_audio_transcript.py:121-335
 * (split_long_audio_kaldifolder) does utterance by utterance through compute_alignment.  Padded layouts: emission
 * [B, Fmax, V], frame_lens [B] (NULL = Fmax), tokens [B, Lmax], token_lens [B] (NULL = Lmax), col0 [B, Fmax+1] or NULL,
 * trellis [B, Fmax+1, Lmax+1] or NULL (utterance b fills the top-left (F_b+1) x (L_b+1) corner; callers that only cut audio
 * at word boundaries do not need it), path_token / path_logp [B, Fmax], path_info [B, 2] (as above; -3 = a length outside
 * [1, Fmax] / [1, Lmax]).  Every utterance's results are bit-identical to its single-utterance call. */
size_t ssak_ctc_align_batch_workspace_bytes(int B, int Fmax, int Lmax);
int ssak_ctc_forced_align_batch(const float* emission, const int32_t* frame_lens, const int32_t* tokens, const int32_t* token_lens,
                                int B, int Fmax, int V, int Lmax, int blank, const float* col0, float* trellis, int32_t* path_token,
                                float* path_logp, int32_t* path_info /*[B,2]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- dense contraction (MFMA bf16, fp32 accumulate) -----------------------------------------
 * The one GEMM behind every Linear / Conv1d / attention product of a3-a10.  C = alpha * op(A) * op(B)
 * (+ epilogue).  Operand layouts: *_kmajor = 0 -> stored [rows, K] with K contiguous (A: [M,K], B: [N,K],
 * i.e. an nn.Linear weight); 1 -> stored [K, rows] (A: [K,M], B: [K,N]).  ld* are element strides of the
 * stored matrix (multiples of 8; ldA < K is allowed and gives the overlapping-row "Toeplitz" operand that
 * makes a channels-last Conv1d a plain GEMM).  Two batch levels: z = z1 * nb2 + z2 with element
 * strides s?1 / s?2 per operand.  Epilogue: bias (fp32 [N] or NULL), then `epilogue` selects
 * NONE / GELU (optionally saving the pre-activation to `aux_out`) / MUL_GELU_GRAD (C *= gelu'(aux_in)).
 * out_f32 selects fp32 vs bf16 C.  split_k > 1 needs workspace >= split_k*batch*M*N*4 bytes and is summed
 * deterministically by a second kernel; split_k = 0 lets the library size the split (<= 32, and only as far as
 * `workspace_bytes` allows; plain epilogue only, otherwise 1) -- the weight-gradient form, long K and few tiles. */
#define SSAK_EPI_NONE 0
#define SSAK_EPI_GELU 1
#define SSAK_EPI_MUL_GELU_GRAD 2
/* The feed-forward pair of the encoder layers (Wav2Vec2FeedForward, modeling_wav2vec2.py:565-572, and its autograd): the
 * forward GEMM computes y = dropout(gelu(x)) and, instead of the pre-activation x, saves the backward's whole elementwise
 * factor f = gelu'(x) * keep / (1 - p) to `aux_out` (same element offsets as C); the backward GEMM then only multiplies,
 * C *= aux_in -- no exp, no reciprocal and no mask hash in the epilogue that used to be the slowest of the layer.
 * ssak_gemm_bf16 stores the factor as ONE BYTE per element (aux buffers are uint8 [.., ldc]): code 26 = exactly 0 (also a
 * dropped element), otherwise gelu'(x) on the uniform grid (code - 26) * 1.26 / 254 over [-0.129, 1.136] (rounding error
 * <= 0.0025, bf16's own error for |f| >= 0.6); 1 / (1 - p) is applied when the codes are read, so the SSAK_EPI_MUL_AUX product
 * is given the forward's drop_p (it draws no mask).  ssak_gemm_f32 keeps a float factor with mask and scale folded in. */
#define SSAK_EPI_GELU_SAVE_GRAD 3
#define SSAK_EPI_MUL_AUX 4
typedef struct {
  int M, N, K;
  int a_kmajor, b_kmajor;
  long lda, ldb, ldc;
  int nb1, nb2;
  long sa1, sa2, sb1, sb2, sc1, sc2;
  float alpha;
  int epilogue;
  int out_f32;
  int accumulate; /* C += result (fp32 out only) */
  int split_k;
  float drop_p;        /* > 0: dropout fused into the epilogue (after GELU / on the GELU-grad product) */
  uint32_t drop_stream; /* keep(drop_seed, drop_stream, output row z * M + m, output column n): replayable in backward */
  uint64_t drop_seed;
  long bias_s2; /* bias element stride per second-level batch index (grouped conv: one bias slice per group) */
  int pads_are_zero; /* caller guarantees that elements between the logical extent and the next multiple of 8
                        (K for K-contiguous operands, rows for K-major ones) are zero in memory: lets operands whose
                        extent is not a multiple of 8 (e.g. 499 frames) take the direct-to-LDS path */
  int colsum; /* != 0: `aux_out` is a float [N] vector that receives += the column sums of the stored C (after the epilogue:
                 the bias gradient of the Linear that produced the GEMM's A operand side), summed in a fixed order;
                 needs workspace >= ceil(M / 64) * N * 4 bytes; not with SSAK_EPI_GELU, split_k or batches */
  int dynamic_tiles; /* tile order of the persistent kernels for THIS product.  0 (default): static stride over the workgroups;
                 1: every tile is drawn from per-XCD ticket counters, so that workgroups whose CU is held by another stream's
                 kernel for a while -- the RCCL all-reduce of a data-parallel step -- take fewer tiles instead of finishing
                 last.  Alone on the chip the static order is a few percent faster (no ticket round trip at the start of a
                 launch); results are bit-identical either way.  (A grouped launch reads it from descs[0].) */
  const void* b_fragments; /* optional (NULL = none): the FRAGMENT-ORDERED copy of this product's B operand made by
                 ssak_gemm_fragment_b for the same N, K -- for a B that is a weight, static between optimizer steps.  When the
                 library picks the persistent kernel's "B-direct" form for the shape (ssak_gemm_uses_fragments), every wave
                 loads its B fragments from this copy straight into registers and B never enters LDS (the LDS form is bound by
                 LDS read bandwidth; N = 768 products of the train step run 5-25 % faster); otherwise it is ignored and B is
                 read.  Both must describe the same matrix: results are bit-identical either way.  Not with B batch strides. */
  int plan_tile; /* 0 (default): the library's cost model picks kernel, tile height and split.  256 / 192 / 128: run the product
                 on the persistent 256-column-tile kernels with this tile height whenever it qualifies for them (M, N >= 256,
                 whole 16-byte chunks) -- for tests and tuning; results do not depend on it beyond the summation order.  (Round 5's
                 value 129, a co-resident 128-row-tile kernel that never won a shape, is gone: tools/probes/gemm_c4.hip.txt.) */
} ssak_gemm_desc;
/* Fragment-ordered copy of a B operand ([N, K] K-contiguous, or [K, N] with b_kmajor; ldb as in the descriptor):
 * out[(cb * nkt + kt)][j][kk][lane][8] = B(n = 64 cb + 16 j + (lane & 15), k = 64 kt + 32 kk + 8 (lane >> 4) + e), zeros
 * beyond N / K, cb < 4 * ceil(N / 256), nkt = ceil(K / 64): the 8 KB one wave column needs for one 64-deep K tile are
 * contiguous and each `v_mfma_f32_16x16x32_bf16` operand is one 1-KiB wave-level load of whole cache lines. */
size_t ssak_gemm_fragment_b_bytes(int N, int K);
int ssak_gemm_fragment_b(const void* B, long ldb, int N, int K, int b_kmajor, void* out, void* stream);
/* The same for `n` matrices in ONE launch (host arrays of length n): the engine refreshes the copies of every kept layer's
 * weights once per train step. */
int ssak_gemm_fragment_b_batched(int n, const void* const* B, const long* ldb, const int* N, const int* K, const int* b_kmajor,
                                 void* const* out, void* stream);
/* 1 when ssak_gemm_bf16 would take the B-direct form for this descriptor if b_fragments were given (callers that keep the
 * copies fresh only for products that use them), else 0. */
int ssak_gemm_uses_fragments(const ssak_gemm_desc* desc);
int ssak_gemm_bf16(const ssak_gemm_desc* desc /*host*/, const void* A, const void* B, void* C, const float* bias,
                   const void* aux_in, void* aux_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same contraction with float operands, float results and float aux buffers on the fp32 matrix pipe
 * (v_mfma_f32_32x32x2_f32): the GEMM of the fp32-exact verification mode (ssak_w2v2_config.exact).  The reference computes
 * these products in fp32 (USE_MIXED_PRECISION = False, ssak/train/transformers/wav2vec_train.py:191-192).  out_f32, split_k,
 * pads_are_zero are ignored (always float, never split, every access bounds-checked); colsum adds with float atomics. */
int ssak_gemm_f32(const ssak_gemm_desc* desc /*host*/, const void* A, const void* B, void* C, const float* bias,
                  const void* aux_in, void* aux_out, void* stream);

/* Grouped form: n <= 48 plain products (no bias / activation / dropout / batches / split-K) that share K, the operand layouts,
 * alpha and the output type run as ONE persistent launch whose tiles are dealt over the whole chip -- the weight gradients
 * dW = dY^T X of the encoder layers (loss.backward() of wav2vec_train.py:415), which one at a time are too few tiles to fill
 * the GPU without split-K slabs: the engine launches two layers at a time (216 tiles, one round; under data parallelism their
 * gradient ranges become ready early for the all-reduce).  descs / A / B / C are host arrays of length n. */
int ssak_gemm_bf16_grouped(const ssak_gemm_desc* descs /*host*/, int n, const void* const* A, const void* const* B, void* const* C,
                           void* stream);

/* Per-launch timing for the roofline report (measurement aid, not on the reference's path): while enabled, launches are
 * bracketed by HIP events on their own stream; ssak_prof_collect waits for them and returns one entry per slot: the kernel
 * classes of the train step (attention, LayerNorm, conv0, AdamW, CTC, ...) and every GEMM instantiation launched so far
 * (named as rocprofv3 prints it), each with launches / summed ms / ALGORITHMIC work -- flops for SSAK_BOUND_MFMA slots,
 * bytes for SSAK_BOUND_HBM / SSAK_BOUND_LATENCY slots.  Timing is switched on PER STREAM (no process-wide state: launches on
 * other streams -- another handle, another thread -- are not touched and not reported): ssak_prof_enable(stream, 0) = off,
 * (stream, 1) = every launch on that stream, (stream, 2 + i) = only slot i:
 * an event pair keeps consecutive kernels from overlapping head to tail, and bracketing all launches of a train step costs
 * a few per cent of it, so a benchmark surveys all slots in warm-up steps and times only the slot it reports on inside its
 * timed region. */
#define SSAK_BOUND_MFMA 0
#define SSAK_BOUND_HBM 1
#define SSAK_BOUND_LATENCY 2
typedef struct {
  char name[112];
  long launches;
  double total_ms;
  double total_flops; /* flops, or bytes for the HBM / latency-bound slots */
  int bound;
} ssak_prof_entry;
int ssak_prof_enable(void* stream, int on);
/* as ssak_prof_enable(stream, 2 + i) for a LIST of slots (indices into ssak_prof_collect's list): a kernel that serves several
 * products has one slot per (N, K); a benchmark that reports on the kernel times all of them. */
int ssak_prof_enable_slots(void* stream, const int32_t* slots, int n);
int ssak_prof_collect(void* stream, ssak_prof_entry* out /*host*/, int cap); /* cap >= 128; returns the number of entries */

/* ---- a3 (part): first layer of the feature encoder -------------------------------------------
 * Conv1d(1, C, k=10, s=5, no bias) -> GroupNorm(C groups: per channel over time) -> GELU of Wav2Vec2GroupNormConvLayer
 * (transformers modeling_wav2vec2.py:302-323), waveform x [B, T] fp32 -> out [B, T0, C] bf16 channels-last, T0 = (T-10)/5+1.
 * w [C, 10], gamma / beta [C] fp32.  Statistics in fp64 from 65 input moments per utterance; for C = 512 the taps run on the
 * matrix cores with a three-term bf16 split (fp32-grade).  Exported for per-op parity tests; the engine calls the same code. */
size_t ssak_conv0_workspace_bytes(int B, int T, int C);
int ssak_conv0_gn_gelu(const float* x, const float* w, const float* gamma, const float* beta, void* out_bf16, void* workspace,
                       size_t workspace_bytes, int B, int T, int C, void* stream);
/* the same on RAW full-length waveforms, the zero-mean / unit-variance normalisation folded into the GroupNorm statistics:
 * out == ssak_conv0_gn_gelu(ssak_wave_normalize(x)) to fp32 rounding (SSAK_W2V2_OPT_RAW_INPUT uses it) */
int ssak_conv0_gn_gelu_raw(const float* x, const float* w, const float* gamma, const float* beta, void* out_bf16, void* workspace,
                       size_t workspace_bytes, int B, int T, int C, void* stream);

/* ---- a7 (part): fused self-attention, head_dim 64 --------------------------------------------
 * Replaces Wav2Vec2Attention's softmax(QK^T d^-0.5 + key mask) -> dropout -> .V and its autograd
 * (transformers modeling_wav2vec2.py:438-463,500-548) for one layer.  qkv [B*F, 3H] bf16 (q | k | v, heads
 * interleaved in the channel dimension), ctx [B*F, H] bf16, lse [B, nh, F] fp32 (saved for the backward),
 * klens [B] valid keys or NULL.  Backward: dctx [B*F, H] -> dqkv [B*F, 3H]; delta [B, nh, F] fp32 scratch.
 * Exported for per-op parity tests; the engine calls the same kernels. */
int ssak_attention_fwd(const void* qkv, void* ctx, float* lse, const int32_t* klens, int B, int F, int nh, int H, float drop_p,
                       uint64_t seed, uint32_t stream_id, void* stream);
int ssak_attention_bwd(const void* qkv, const void* ctx, const float* lse, const int32_t* klens, const void* dctx, float* delta,
                       void* dqkv, int B, int F, int nh, int H, float drop_p, uint64_t seed, uint32_t stream_id, int mode,
                       void* stream);
/* `mode` of the backward: SSAK_ATTN_BWD_DEFAULT = SSAK_ATTN_BWD_TWO_KERNEL = two kernels (dQ; dK + dV), each recomputing P from the
 * saved log-sum-exp.  (Value 2, a fused single-pass form that lost to this one at the train step's shape, was removed in ABI 400:
 * SSAK_ERR_ARG.) */
#define SSAK_ATTN_BWD_DEFAULT 0
#define SSAK_ATTN_BWD_TWO_KERNEL 1
/* As ssak_attention_bwd, and bias_grad[3H] += the column sums of dqkv -- the gradient of the q|k|v projection bias (the Linear layers
 * of Wav2Vec2Attention, modeling_wav2vec2.py:500-548) -- summed inside the two kernels from the rows they hold (deterministic: one
 * partial row per workgroup in `workspace`, one fixed-order second stage), instead of a pass that reads dqkv again. */
size_t ssak_attention_bwd_bias_workspace_bytes(int B, int F, int H);
int ssak_attention_bwd_bias(const void* qkv, const void* ctx, const float* lse, const int32_t* klens, const void* dctx, float* delta,
                            void* dqkv, float* bias_grad, int B, int F, int nh, int H, float drop_p, uint64_t seed,
                            uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a11: optimizer tail (clip_grad_norm_ -> AdamW), flat fp32 buffers ----------------------
 * Replaces torch.nn.utils.clip_grad_norm_(max 1.0) + torch.optim.AdamW.step as driven by HF Trainer
 * (docker/transformers_modified/trainer.py:1827-1855; ssak/train/transformers/wav2vec_train.py:353-384).
 * ssak_grad_sumsq: out[0] = sum(grads^2), summed in a fixed order (per-workgroup partials in `workspace`, >= 4096 bytes,
 * then one pass): the clip coefficient is reproducible run to run.  ssak_adamw_step: g' = grads * grad_scale * min(1, max_norm /
 * (sqrt(gnorm_sq[0]) * grad_scale + 1e-6)) (no clipping when gnorm_sq is NULL or max_norm <= 0), then the
 * AdamW update with bias correction for 1-based `step`; shadow_bf16 (or NULL) receives the bf16 copy of the
 * new parameters.  The clip coefficient is read on the device: no host synchronisation. */
int ssak_grad_sumsq(const float* grads, long n, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* out[0] += sum g^2: the joint norm over several buffers (the SpeechBrain recipe clips the wav2vec2 and head gradients as one
 * vector, speechbrain core Brain.check_gradients under ssak/train/speechbrain/wav2vec_train.py:113,125) */
int ssak_grad_sumsq_add(const float* grads, long n, float* out, void* workspace, size_t workspace_bytes, void* stream);
int ssak_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, long n,
                    const float* gnorm_sq, float max_norm, float grad_scale, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, void* stream);

/* ---- e: data-parallel gradient exchange ------------------------------------------------------
 * One process per GPU, utterance shards per rank, ONE sum all-reduce of the flat gradient buffer per step (in buckets, as the
 * backward announces them: ssak_w2v2_set_grad_ready_callback) -- what torch.nn.DataParallel's gather + loss.mean() does inside
 * HF Trainer for the reference (docker/transformers_modified/trainer.py:2532-2533; per_device_train_batch_size = batch_size //
 * num_devices, ssak/train/transformers/wav2vec_train.py:349,356).  RCCL over xGMI; librccl.so is dlopen'ed on the first call
 * (libssak_hip.so does not link it: a single-GPU host never loads it).  Rank 0 calls ssak_comm_unique_id and hands the 128
 * bytes to the other ranks by its own means (file, socket, MPI, torch.distributed); every rank then calls ssak_comm_create
 * (collective).  ssak_allreduce: buf[offset, offset + count) of `dtype` elements := the sum over ranks, in place, asynchronous
 * on `stream`; 1 / world is folded into ssak_adamw_step's grad_scale.  One communicator per process and device. */
typedef struct ssak_comm ssak_comm;
#define SSAK_DTYPE_F32 0
#define SSAK_DTYPE_BF16 1
int ssak_comm_unique_id(void* id128 /*host, 128 bytes out*/);
int ssak_comm_create(ssak_comm** out, int world, int rank, const void* id128 /*host*/);
int ssak_allreduce(ssak_comm* comm, void* buf, long offset, long count, int dtype, void* stream);
int ssak_comm_destroy(ssak_comm* comm);

/* ---- a3-a10: the Wav2Vec2-CTC acoustic model ------------------------------------------------
 * Replaces `model(input_values, attention_mask, labels)` / `loss.backward()` of transformers.Wav2Vec2ForCTC as
 * called at ssak/train/transformers/wav2vec_train.py:387-415 (through HF Trainer.training_step) and
 * ssak/infer/transformers_infer.py:235.  The handle owns only derived weight layouts; parameters, gradients,
 * the bf16 shadow and the workspace are caller-owned flat device buffers.
 *
 * Parameter layout: ssak_w2v2_param_info enumerates (HF state_dict name, element offset, shape) of every
 * tensor inside the flat buffers; [0, ssak_w2v2_num_trainable) is what the optimizer / all-reduce touch. */
typedef struct {
  int vocab_size, hidden_size, num_layers, num_heads, intermediate_size;
  int num_conv_layers;
  int conv_dim[8], conv_kernel[8], conv_stride[8];
  int conv_bias;            /* 0 (base) */
  int feat_extract_norm;    /* 0 = "group" (base), 1 = "layer" (XLSR) */
  int do_stable_layer_norm; /* 0 = post-LN (base) */
  int num_conv_pos_embeddings, num_conv_pos_embedding_groups;
  float layer_norm_eps;
  float attention_dropout, hidden_dropout, activation_dropout, feat_proj_dropout, final_dropout;
  int freeze_feature_encoder; /* wav2vec_train.py:326-327 */
  /* arch 1 = Whisper encoder + CTC head (BASELINE config 4; a composition of the build): conv1/conv2
   * front end on log-mel features, fixed sinusoidal positions, pre-LN layers (k_proj without bias), final LayerNorm,
   * Linear(d_model, vocab).  input_values is then the feature tensor [B, num_mel_bins, T] (T = 2 * frames, even). */
  int arch;
  int num_mel_bins, max_source_positions;
  /* exact != 0: the fp32-exact VERIFICATION mode -- activations are stored in float, every product runs through
   * ssak_gemm_f32 on the fp32 master weights, GELU is the exact erf form, attention takes the unfused GEMM + softmax path;
   * the engine's sequencing, layouts, row kernels (the same templates as the bf16 mode) and the CTC kernels are then
   * comparable with the fp32 reference at 1e-4 instead of bf16's 1e-2.  wav2vec2 topologies with the frozen feature
   * encoder; a few per cent of the bf16 mode's speed.  Workspace sizes double. */
  int exact;
  /* ABI 590: MMS language adapters (transformers Wav2Vec2AttnAdapterLayer, config.adapter_attn_dim).  0 = none: parameter
   * table, buffer plan and launch sequence are those of ABI 580.  > 0 (16, MMS's value, is the one supported): every encoder
   * layer ends with h = h + W2 relu(W1 LN(h) + b1) + b2 after its feed-forward residual, LN a plain LayerNorm with eps 1e-5
   * whatever layer_norm_eps says; the parameter table gains wav2vec2.encoder.layers.N.adapter_layer.{norm,linear_1,linear_2}.
   * {weight,bias} per layer after lm_head.bias.  Needs arch 0 and do_stable_layer_norm 1 (HF's post-LN layer has no
   * adapter).  Inference only: a training-mode forward and the backward are SSAK_ERR_INVALID on such a handle. */
  int adapter_attn_dim;
} ssak_w2v2_config;
typedef struct ssak_w2v2 ssak_w2v2;

int ssak_w2v2_create(const ssak_w2v2_config* cfg /*host*/, ssak_w2v2** out);
void ssak_w2v2_destroy(ssak_w2v2* h);
long ssak_w2v2_num_params(const ssak_w2v2* h);
long ssak_w2v2_num_trainable(const ssak_w2v2* h);
int ssak_w2v2_param_count(const ssak_w2v2* h);
int ssak_w2v2_param_info(const ssak_w2v2* h, int index, char* name /*host*/, int name_cap, long* offset, long* numel,
                         int* ndim, long* shape4 /*host [4]*/);
/* params/grads fp32 [num_params] (grads may be NULL for inference), shadow_bf16 uint16 [num_params] */
int ssak_w2v2_bind(ssak_w2v2* h, float* params, float* grads, void* shadow_bf16);
/* full != 0: rebuild the whole bf16 shadow + conv layouts from `params` (after loading weights);
 * full == 0: only the weight-normed positional-conv layouts (after an optimizer step that updated the shadow). */
int ssak_w2v2_sync_weights(ssak_w2v2* h, int full, void* stream);
int ssak_w2v2_num_frames(const ssak_w2v2* h, int T); /* floor((L-k)/s)+1 chain, modeling_wav2vec2.py:997-1016 */
size_t ssak_w2v2_workspace_bytes(const ssak_w2v2* h, int B, int T, int training);
/* input_values [B,T] fp32 normalised waveforms; lens [B] int32 valid samples or NULL (= no attention mask, the
 * group-norm/base convention); spec_mask [B,F] uint8 SpecAugment mask or NULL; layer_keep host uint8 [num_layers]
 * LayerDrop decisions or NULL; seed drives every dropout mask of this step; logits [B,F,V] fp32 out;
 * frame_lens [B] int32 out (or NULL).  training != 0 keeps the activations for ssak_w2v2_backward. */
int ssak_w2v2_forward(ssak_w2v2* h, const float* input_values, const int32_t* lens, int B, int T,
                      const uint8_t* spec_mask, const uint8_t* layer_keep /*host*/, uint64_t seed, int training,
                      float* logits, int32_t* frame_lens, void* workspace, size_t workspace_bytes, void* stream);
/* Optional: called (on the host, from inside ssak_w2v2_backward) each time all kernels writing a contiguous range
 * grads[offset, offset+count) have been enqueued on the stream -- once per encoder layer (top to bottom), then for
 * the rest.  The ranges are disjoint and cover [0, num_trainable).  A data-parallel caller launches one bucketed
 * all-reduce per announcement on a side stream so that the exchange overlaps the remaining backward
 * (the reference's nn.DataParallel reduces after backward, docker/transformers_modified/trainer.py:1345-1346). */
typedef void (*ssak_grad_ready_fn)(long offset, long count, void* user);
int ssak_w2v2_set_grad_ready_callback(ssak_w2v2* h, ssak_grad_ready_fn fn, void* user);
/* Optimizer on a side stream (north_star: "all-reduce ... overlapped with the optimizer on a side HIP stream"; the reference's
 * HF Trainer runs optimizer.step() in line, docker/transformers_modified/trainer.py:1827-1855): `params_ready` is a hipEvent_t the
 * caller records on its optimizer stream after the update of params / shadow (and ssak_w2v2_sync_weights(full = 0)) has been
 * enqueued there.  Every forward then waits for it on ITS stream at the first kernel that reads a trainable parameter -- with
 * a frozen feature encoder that is the feature projection, so the whole conv stack of step n+1 runs under the exchange tail and
 * the AdamW sweep of step n.  stall_begin / stall_end (hipEvent_t or NULL) are recorded around that wait: their distance is the
 * exposed part of the tail.  NULL params_ready removes the wait. */
int ssak_w2v2_set_param_event(ssak_w2v2* h, void* params_ready, void* stall_begin, void* stall_end);
/* Per-handle execution options (nothing here changes results beyond rounding; no process-wide switches):
 * SSAK_W2V2_OPT_DYNAMIC_TILES  0 / 1: ssak_gemm_desc.dynamic_tiles of every product the engine launches -- the data-parallel
 *                              trainers set it, RCCL's kernels share the chip with the persistent GEMMs;
 * SSAK_W2V2_OPT_ATTENTION_BWD  SSAK_ATTN_BWD_* (one form since ABI 400; kept so that callers need not change);
 * SSAK_W2V2_OPT_POSCONV_DIRECT  1 (default) / 0: the grouped positional convolution (forward, input gradient and weight gradient)
 *                              as direct convolutions with the input rows resident in LDS (group widths 48 and 64) or as the
 *                              Toeplitz GEMMs of rounds 1-2 (kept for other geometries and as the comparison path of the tests);
 * SSAK_W2V2_OPT_FRAGMENT_WEIGHTS  0 (default) / 1: every TRAINING forward makes fragment-ordered copies of the kept encoder
 *                              layers' projection weights (one batched launch after the optimizer's event, ssak_gemm_fragment_b)
 *                              and the forward / input-gradient products the library would run in its B-direct form take
 *                              them through ssak_gemm_desc.b_fragments; evaluation forwards never do (the copies would go
 *                              stale when the caller rewrites the shadow).  Bit-identical results; engine-owned memory (~2 x
 *                              the bf16 size of the layers' matrices).  OFF by default: with the operands warm the B-direct
 *                              form is 5-25 % faster on the N = 768 products, but in the train step a layer's weights are read
 *                              once per step -- from HBM -- and the gain is gone (3 591 -> 3 664 us per step for the six
 *                              products, + 160 us for the copies: profiles/r03_ab_fragments.log);
 * SSAK_W2V2_OPT_TRANSPOSED_WEIGHTS  1 (default) / 0: every TRAINING forward makes TRANSPOSED bf16 copies of the kept encoder layers'
 *                              four projection matrices (one batched launch after the optimizer's event, ~310 MB of traffic for
 *                              wav2vec2-base) and the backward's input-gradient products dX = dY W read them as a K-contiguous
 *                              B operand -- the layout of the four-wave GEMM (gemm_p4.hip) -- instead of the weight itself
 *                              K-major.  Same products, summation order aside; engine-owned memory (the bf16 size of the
 *                              layers' matrices).  Used when hidden and intermediate sizes are multiples of 256. */
#define SSAK_W2V2_OPT_DYNAMIC_TILES 1
#define SSAK_W2V2_OPT_ATTENTION_BWD 2
#define SSAK_W2V2_OPT_POSCONV_DIRECT 3
#define SSAK_W2V2_OPT_FRAGMENT_WEIGHTS 4
#define SSAK_W2V2_OPT_TRANSPOSED_WEIGHTS 5
/* SSAK_W2V2_OPT_RAW_INPUT  0 (default) / 1: `input_values` of ssak_w2v2_forward are RAW full-length waveforms (no padding inside the
 * batch): the feature extractor's zero-mean / unit-variance normalisation (a1, ssak/utils/dataset.py:632) is folded into the
 * GroupNorm statistics of the first conv layer -- conv0 is linear and bias-free, so only GroupNorm's epsilon changes (1e-5 sigma^2) --
 * and the train step needs no ssak_wave_normalize pass.  wav2vec2 group-norm feature encoder, frozen, only; logits equal the
 * two-pass form's to fp32 rounding.  Ragged batches and inference keep ssak_wave_normalize. */
#define SSAK_W2V2_OPT_RAW_INPUT 6
int ssak_w2v2_set_option(ssak_w2v2* h, int option, int value);
/* The gradient ranges ssak_w2v2_backward announces, in announcement order, from the configuration alone (host arithmetic, no
 * device): head matrix, one range per encoder layer from the last to the first (a layer's q|k|v|out|ffn matrices are
 * contiguous), the leading small matrices, then the vector region (biases, LayerNorm affines) [+ the feature encoder when it
 * is trained].  They are disjoint, start at multiples of 8 elements and cover [0, num_trainable): the buckets of the
 * data-parallel exchange.  Returns the number of ranges (<= cap written), negative on a bad configuration. */
int ssak_w2v2_grad_ranges(const ssak_w2v2_config* cfg /*host*/, long* offsets /*host*/, long* counts /*host*/, int cap);
/* dlogits [B,F,V] fp32 (e.g. from ssak_ctc_loss_fwd_bwd); overwrites grads[0, num_trainable). */
int ssak_w2v2_backward(ssak_w2v2* h, const float* dlogits, void* workspace, size_t workspace_bytes, void* stream);
/* The same model stopped at the encoder's last hidden state -- `self.modules.wav2vec2(wavs)` of the SpeechBrain recipe
 * (ssak/train/speechbrain/wav2vec_train.py:51; HuggingFaceWav2Vec2 returns Wav2Vec2Model(wav)[0]): hidden [B,F,H] bf16 out, no
 * final dropout, no lm_head.  ssak_w2v2_backward_hidden continues from d loss / d hidden [B,F,H] bf16 (the unfrozen case,
 * :95-137); the lm_head gradient stays zero.  A backward must match the kind of forward that preceded it.  In the fp32-exact
 * mode (since ABI 580; refused before) hidden and dhidden are float [B,F,H], the engine's storage type in that mode. */
int ssak_w2v2_forward_hidden(ssak_w2v2* h, const float* input_values, const int32_t* lens, int B, int T,
                             const uint8_t* spec_mask, const uint8_t* layer_keep /*host*/, uint64_t seed, int training,
                             void* hidden_bf16, int32_t* frame_lens, void* workspace, size_t workspace_bytes, void* stream);
int ssak_w2v2_backward_hidden(ssak_w2v2* h, const void* dhidden_bf16, void* workspace, size_t workspace_bytes, void* stream);

/* ---- f4: the SpeechBrain recipe's acoustic head ------------------------------------------------
 * Row-wise pieces of `x = enc(feats); logits = ctc_lin(x)` (ssak/train/speechbrain/wav2vec_train.py:51-54) with the modules
 * of ssak/train/speechbrain/fr/hyperparameters_wav2vec_finetune_cv-fr.yaml:87-137; the Linears are ssak_gemm_bf16, log-softmax
 * + ctc_cost is ssak_ctc_loss_fwd_bwd.  Host-side composition: ssak_amd/sb_head.py.
 *
 * ssak_utt_norm_*: F.layer_norm(x, x.shape[1:]) without affine parameters -- the wrapper's waveform normalisation (fp32,
 * is_bf16 = 0) and its output_norm over (frames x features) (bf16, is_bf16 = 1).  x, y [B, n]; stats [B][2] = (mean, rstd) out
 * (may be NULL in the forward when no backward follows); the backward takes y, the forward's OUTPUT.  Any n (rows whose length
 * is a multiple of 8 bf16 / 4 fp32 elements take the 16-byte vector path). */
size_t ssak_utt_norm_workspace_bytes(int B);
int ssak_utt_norm_fwd(const void* x, void* y, int B, long n, int is_bf16, float eps, float* stats, void* workspace,
                      size_t workspace_bytes, void* stream);
int ssak_utt_norm_bwd(const void* dy, const void* y, void* dx, int B, long n, int is_bf16, const float* stats, void* workspace,
                      size_t workspace_bytes, void* stream);
/* BatchNorm1d over all M = B*T rows of x [M, C] bf16 (speechbrain BatchNorm1d on [B,T,C]: statistics over batch and time,
 * padding frames included), then LeakyReLU(leaky_slope) and dropout(drop_p), one fused apply pass: y [M, C] bf16.
 * training != 0: batch statistics (biased variance), running_mean / running_var (or NULL) updated with `momentum` and the
 * unbiased variance; training == 0: the running statistics, no dropout.  save_mean / save_rstd [C] out are what the backward
 * needs together with x.  Backward: dy -> dx, dgamma / dbeta [C] overwritten; the dropout mask is recomputed from
 * (seed, drop_stream, element index).  Sums are two-stage and fixed-order (deterministic).  C a multiple of 8. */
size_t ssak_batchnorm_workspace_bytes(int C);
int ssak_batchnorm_act_fwd(const void* x, void* y, int M, int C, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float momentum, float eps, int training, float leaky_slope, float drop_p,
                           uint64_t seed, uint32_t drop_stream, float* save_mean, float* save_rstd, const double* global_sums,
                           void* workspace, size_t workspace_bytes, void* stream);
int ssak_batchnorm_act_bwd(const void* dy, const void* x, void* dx, int M, int C, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_rstd, float leaky_slope, float drop_p, uint64_t seed,
                           uint32_t drop_stream, float* dgamma, float* dbeta, double* local_sums_out, const double* global_sums,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Synchronised statistics under data parallelism (the head's BatchNorm1d spans the global batch): the column
 * totals travel as doubles through one all-reduce of 2 C + 1 values per normalisation and direction (the last one is the
 * row count, so ranks may hold different numbers of rows and no host read is needed).
 *   forward : ssak_batchnorm_stats(x) -> sums[2C+1] = (sum x [C], sum x^2 [C], M) of the local rows; all-reduce(sum);
 *             ssak_batchnorm_act_fwd(..., global_sums = sums)
 *   backward: ssak_batchnorm_act_bwd(dx = NULL, local_sums_out = sums) -> local dgamma / dbeta (the parameter all-reduce sums
 *             them as usual) and sums[2C+1] = (sum g, sum g xhat, M); all-reduce(sum);
 *             ssak_batchnorm_act_bwd(dx, global_sums = sums) -> dx; dgamma / dbeta untouched (may be NULL).
 * With global_sums == NULL and local_sums_out == NULL both calls are the single-device form. */
int ssak_batchnorm_stats(const void* x, int M, int C, double* sums, void* workspace, size_t workspace_bytes, void* stream);
/* torch.optim.Adadelta (yaml :119-122: lr 1.0, rho 0.95, eps 1e-8): square_avg = rho sq + (1-rho) g^2;
 * delta = sqrt(acc_delta + eps) / sqrt(square_avg + eps) * g; acc_delta = rho acc + (1-rho) delta^2; p -= lr * delta.
 * g is first multiplied by grad_scale (1 / world size after a sum all-reduce) and by min(1, max_norm / (sqrt(*gnorm_sq) *
 * grad_scale + 1e-6)) when gnorm_sq != NULL and max_norm > 0 -- the convention of ssak_adamw_step. */
int ssak_adadelta_step(float* params, const float* grads, float* square_avg, float* acc_delta, void* shadow_bf16, long n,
                       const float* gnorm_sq, float max_norm, float grad_scale, float lr, float rho, float eps, float weight_decay,
                       void* stream);
int ssak_cast_f32_bf16(const float* src, void* dst_bf16, long n, void* stream);
/* the way back (the optional bf16 gradient exchange of the data-parallel trainer: 180 MB instead of 361 MB per step,
 * SURVEY.md 8e); 16-byte aligned buffers */
int ssak_cast_bf16_f32(const void* src_bf16, float* dst, long n, void* stream);
/* out[N] = column sums of X [M, N] bf16 (row stride ld): the bias gradient of a Linear from its output gradient.  Two-stage,
 * fixed-order; N and ld multiples of 8. */
size_t ssak_colsum_workspace_bytes(int N);
int ssak_colsum_bf16(const void* X, long ld, int M, int N, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- augmentation (ABI 530): train --data_augment, the reference's SpeechAugment (ssak/utils/augment.py:123-180) -------
 * Contract and draws: ssak_amd/augment.py.  Every parameter is drawn on the host and passed as one fp64 row of SSAK_AUG_NCOL
 * columns per utterance, twice: `params` on the device (read by the kernels) and `params_host`, the same table in host
 * memory (argument validation and launch sizing before any launch).  `lens` / `lens_host` likewise (samples, <= T).
 * Results depend on an utterance's own row and samples only (fixed-order fp64 sums, per-utterance FFT sizes, no atomics). */
#define SSAK_AUG_NONE (-1)
#define SSAK_AUG_GAIN 0      /* y = x * gain_lin                                                          */
#define SSAK_AUG_NOISE_MIX 1 /* y = x + n * (rms(x) / snr_amp) / rms(n), n = the tiled noise segment       */
#define SSAK_AUG_REVERB 2    /* circular convolution with the RIR rotated by its peak, mean|.| rescaled    */
#define SSAK_AUG_KIND 0
#define SSAK_AUG_GAIN_DB 1
#define SSAK_AUG_GAIN_LIN 2    /* 10^(gain_db / 20), computed on the host                                 */
#define SSAK_AUG_SNR_DB 3
#define SSAK_AUG_SNR_AMP 4     /* 10^(snr_db / 20), computed on the host                                  */
#define SSAK_AUG_NOISE 5       /* noise bank entry                                                        */
#define SSAK_AUG_NOISE_START 6 /* first sample of the segment in that entry                               */
#define SSAK_AUG_RIR 7         /* RIR bank entry                                                          */
#define SSAK_AUG_RIR_PEAK 8    /* argmax |h| over the full RIR (first maximum)                            */
#define SSAK_AUG_RATE 9        /* time-stretch rate, [0.5, 2]                                             */
#define SSAK_AUG_OUT_LEN 10    /* round(L / rate) (informative: the device recomputes it)                 */
#define SSAK_AUG_NCOL 11
/* A bank of 1-D fp32 signals (noise files, RIRs) resident on the device: entry i is data[offset[i] .. offset[i] + length[i]).
 * offset / length in device memory, their host mirrors for validation. */
typedef struct ssak_audio_bank {
  int n;
  const float* data;
  const int64_t* offset;
  const int32_t* length;
  const int64_t* offset_host; /* host */
  const int32_t* length_host; /* host */
} ssak_audio_bank;
/* Gain and background noise (rows of kind GAIN / NOISE_MIX; every other row is copied).  x and y [B, T] fp32, may alias.
 * Noise: the segment is entry[start : start + min(L, N)], tiled up to L; rms(n) over the segment before tiling; rms(n) < 1e-9
 * leaves y = x.  Samples past lens[b] are copied. */
size_t ssak_augment_gain_noise_workspace_bytes(int B, int T);
int ssak_augment_gain_noise(const float* x, const int32_t* lens, const int32_t* lens_host /*host*/, int B, int T, const double* params,
                            const double* params_host /*host*/, const ssak_audio_bank* noise /*host struct; may be NULL without NOISE rows*/,
                            float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Reverberation (rows of kind REVERB; every other row is copied).  augment_reverberation.py:104-177: h truncated to its first
 * L samples, rotated by its peak d (d >= L: not rotated), circular convolution of length L, then
 * y = w / (mean|w| + 1e-14) * mean|x|.  Computed as a linear convolution through one complex FFT of x + i h of
 * N = 2^k >= L + min(Lh, L) - 1 points (four-step, N <= 2^24), folded modulo L.  An all-zero x or h[:L] gives y = 0 exactly.
 * x and y may alias.  workspace >= ssak_augment_reverb_workspace_bytes(B, T, longest RIR). */
size_t ssak_augment_reverb_workspace_bytes(int B, int T, int max_rir_len);
int ssak_augment_reverb(const float* x, const int32_t* lens, const int32_t* lens_host /*host*/, int B, int T, const double* params,
                        const double* params_host /*host*/, const ssak_audio_bank* rirs /*host struct; may be NULL without REVERB rows*/,
                        float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Time stretch of every row: librosa.effects.time_stretch(x[:L], rate) (n_fft 2048, hop 512, periodic Hann, centred with
 * zero padding; phase vocoder with its accumulator in fp64; iSTFT of length round(L / rate)).  y [B, T_out] with zeros
 * past out_lens[b] = round(L / rate) (device, may be NULL); y must not alias x.
 * workspace >= ssak_augment_time_stretch_workspace_bytes(B, T, T_out). */
size_t ssak_augment_time_stretch_workspace_bytes(int B, int T, int T_out);
int ssak_augment_time_stretch(const float* x, const int32_t* lens, const int32_t* lens_host /*host*/, int B, int T, const double* params,
                              const double* params_host /*host*/, float* y, int32_t* out_lens, int T_out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- augmentation of the SpeechBrain recipe (ABI 560): TimeDomainSpecAugment's DropFreq and DropChunk in one pass ---------
 * Contract and draws: ssak_amd/augment.py (the project's own, modelled on speechbrain 0.5; parity with speechbrain's bits is
 * unpinned).  The speed perturbation before it is ssak_resample_sinc on the padded batch.
 *   out[b, t] = 0                                        if t lies in one of row b's chunks,
 *             = sum_k taps[k] * x[b, t + k - ntaps / 2]   otherwise (zeros outside [0, T)): a CROSS-CORRELATION, as
 *               torch.nn.functional.conv1d computes it, accumulated in fp32 (any order of the ntaps terms).
 * x, out [B, T] fp32, any T >= 1; out must not overlap x.  taps [ntaps] fp32 on the device, ntaps odd and
 * <= SSAK_AUG_FIR_MAX_TAPS; taps = NULL with ntaps = 0 means no filter (out = x outside the chunks, bit for bit).
 * chunks [B, max_chunks, 2] int32 on the device: (start, end) of the half-open sample ranges to zero, clipped to [0, T) by the
 * kernel; chunk_counts [B] int32 on the device and chunk_counts_host, the same counts in host memory (validated before any
 * launch: 0 <= count <= max_chunks).  chunks = NULL: no chunk is dropped (the counts and max_chunks are then ignored).
 * A workgroup produces SSAK_AUG_FIR_TILE consecutive outputs of one row from a tile plus halo held in LDS; needs no
 * workspace. */
#define SSAK_AUG_FIR_MAX_TAPS 255
#define SSAK_AUG_FIR_TILE 2048
int ssak_augment_fir_drop(const float* x, int B, int T, const float* taps, int ntaps, const int32_t* chunks, const int32_t* chunk_counts,
                          const int32_t* chunk_counts_host /*host*/, int max_chunks, float* out, void* stream);

/* ---- utterance classification on the encoder (ABI 580): pooling, head, loss ------------------------------------------------
 * What ssak/utils/gender.py's Wav2Vec2ForSpeechClassification / HubertForSpeechClassification compute after the encoder
 * (:51-133, :155-237; reached from predict_gender, :242-301): hidden [B, F, H] -> merged_strategy (mean / sum / max over time)
 * -> dropout -> Linear(H, H) -> tanh -> dropout -> Linear(H, C) -> softmax or CrossEntropyLoss, and the autograd of that
 * chain back to d loss / d hidden for ssak_w2v2_backward_hidden.  Host-side composition: ssak_amd/classify.py.  Every sum
 * runs in a fixed order (no float atomics): results are bit-reproducible.  No timing of these kernels has been measured.
 *
 * Pooling.  hidden / dhidden [B, F, H] of `dtype` 0 = bf16 (the engine) or 1 = fp32 (the fp32-exact mode), 16-byte aligned,
 * H a multiple of 8, B <= 65535.  frame_lens [B] int32 on the device and frame_lens_host, THE SAME VALUES in host memory
 * (validated before any launch: 1 <= len <= F, so a zero length is SSAK_ERR_INVALID) -- both or neither; NULL pools all F
 * frames, padding included: the reference's torch.mean(hidden, dim=1).  With lengths only frames < len are pooled and mean
 * divides by len.  pooled [B, H] fp32; max also writes argmax [B, H] int32, the LOWEST frame that attains the maximum (NULL
 * for the other modes).  The host copy is what is CHECKED and the device copy is what the kernels READ: a binder keeps one
 * source for both.  Should they disagree, nothing faults -- the kernels clamp a device length into [0, F] (a row of length 0
 * pools to 0, or to -inf under max, with argmax 0) and a device label outside [0, C) gives a NaN loss -- but the result is not the checked one.
 * Backward: dhidden is written whole -- dpooled / len (mean), dpooled (sum) or dpooled at the argmax
 * frame (max), exact zeros at frames >= len and everywhere else. */
#define SSAK_POOL_MEAN 0
#define SSAK_POOL_SUM 1
#define SSAK_POOL_MAX 2
int ssak_pool_fwd(const void* hidden, const int32_t* frame_lens, const int32_t* frame_lens_host /*host*/, int B, int F, int H, int mode,
                  int dtype, float* pooled, int32_t* argmax, void* stream);
int ssak_pool_bwd(const float* dpooled, const int32_t* argmax, const int32_t* frame_lens, const int32_t* frame_lens_host /*host*/, int B,
                  int F, int H, int mode, int dtype, void* dhidden, void* stream);
/* The head, all fp32: z = drop(pooled) W1^T + b1, act = tanh(z) [B, H] (saved for the backward), logits = drop(act) W2^T + b2
 * [B, C]; W1 [H, H], b1 [H], W2 [C, H], b2 [C] as nn.Linear stores them; H a multiple of 4, matrices and activations 16-byte
 * aligned.  Both dropouts use probability drop_p under `seed` with the library's counter-based mask on the sites below, (row,
 * col) = (utterance, feature) of the [B, H] tensor: ssak_debug_dropout_mask(seed, site, drop_p, B, H) reproduces them.
 * training == 0 or drop_p == 0: no dropout.  Backward (same drop_p / seed / training as the forward): dW1, db1, dW2, db2
 * OVERWRITTEN, dpooled [B, H]; workspace >= ssak_cls_head_bwd_workspace_bytes, 16-byte aligned. */
#define SSAK_CLS_SITE_INPUT 4  /* dropout of the pooled vector, in front of `dense` */
#define SSAK_CLS_SITE_HIDDEN 5 /* dropout of tanh(dense), in front of `out_proj` */
int ssak_cls_head_fwd(const float* pooled, const float* W1, const float* b1, const float* W2, const float* b2, int B, int H, int C,
                      float drop_p, uint64_t seed, int training, float* act, float* logits, void* stream);
size_t ssak_cls_head_bwd_workspace_bytes(int B, int H, int C);
int ssak_cls_head_bwd(const float* dlogits, const float* pooled, const float* act, const float* W1, const float* W2, int B, int H, int C,
                      float drop_p, uint64_t seed, int training, float* dW1, float* db1, float* dW2, float* db2, float* dpooled,
                      void* workspace, size_t workspace_bytes, void* stream);
/* probs [B, C] = softmax(logits).  With labels [B] int32 (device) and labels_host (the same values in host memory, validated
 * before the launch: a label outside [0, C) is SSAK_ERR_INVALID) -- both or neither -- also loss [1] = the mean over the batch
 * of -log probs[b, label_b] (CrossEntropyLoss, gender.py:117-119) and dlogits [B, C] = (probs - onehot) / B * grad_scale;
 * either may be NULL.  Without labels loss and dlogits must be NULL. */
int ssak_cls_softmax_ce(const float* logits, const int32_t* labels, const int32_t* labels_host /*host*/, int B, int C, float grad_scale,
                        float* probs, float* loss, float* dlogits, void* stream);

/* ---- the Whisper text decoder (ABI 600): embedding, attention, per-row log-softmax statistics ------------------------------
 * The decoder of transformers' WhisperForConditionalGeneration as a teacher-forced pass (ssak/infer/whisper_infer.py and
 * ssak/train/transformers/whisper_train.py:498-507 run it): these three entries plus ssak_gemm_bf16 (projections, feed-forward,
 * the vocabulary projection against the tied embedding) and ssak_layernorm_fwd.  Host-side composition:
 * ssak_amd/whisper_seq2seq.py.  bf16 storage, fp32 accumulation; every sum in a fixed order, no float atomics; nothing is saved (the
 * backward is ABI 650 below).  No per-kernel timing has been measured (whole calls: tools/bench_whisper_decoder.py).
 *
 * ssak_dec_embed.  out [B * L, D] bf16, out[b, i, :] = bf16(fp32(embed_tokens[ids[b, i], :]) + fp32(embed_positions[pos_offset +
 * i, :])); embed_tokens [V, D] and embed_positions [max_positions, D] bf16, D a multiple of 8, all 16-byte aligned.  ids [B * L]
 * int32 on the device and ids_host, THE SAME VALUES in host memory: the host copy is what is checked (an id outside [0, V), or
 * pos_offset + L > max_positions, is SSAK_ERR_INVALID and nothing is launched), the device copy is what the kernel reads (and
 * clamps into the table, should the two disagree).
 *
 * ssak_dec_attention_fwd.  ctx [B * Lq, nh * 64] bf16 = softmax(q k^T * 64^-1/2 + mask) v per (utterance, head), the scaling
 * applied to q (transformers' WhisperAttention).  q [B * Lq, ldq]; k and v are SEPARATE pointers with row strides ldk / ldv and
 * Lk rows per utterance (utterance b's key j is row b * Lk + j), head h in columns [64 h, 64 h + 64) of each: self-attention
 * points q, k, v into one packed [B * L, 3 D] buffer (ld = 3 D, Lk = Lq), cross-attention points k, v into the encoder-side
 * [B * S, 2 D] buffer.  Strides are in elements, multiples of 8 and >= nh * 64; pointers 16-byte aligned.  Visibility: key j is
 * visible to query i iff j < klens[b] and, when causal != 0, j <= q_offset + i (q_offset: the position of the first query
 * among the keys -- 0 for a whole sequence, the cache length for an incremental step).  klens [B] int32 (device) and klens_host
 * (host, the same values) come together or are both NULL (= Lk); the host copy is validated, 1 <= klens[b] <= Lk, so a fully
 * masked row cannot occur (causal always shows key 0).  head_dim must be 64, the head dimension of every Whisper size: any
 * other value is SSAK_ERR_INVALID.  P is rounded to bf16 for the second product; the row sum is that of the unrounded P.
 *
 * ssak_token_logprobs.  Per row r of logits [R, ldv] (dtype 1 = fp32, 0 = bf16; V valid columns, ldv >= V; columns >= V are
 * never read): lse[r] = log sum_c exp(logits[r, c]); logprob[r] = logits[r, targets[r]] - lse[r], 0 where targets[r] < 0 (HF's
 * -100); argmax[r] = the LOWEST column that attains the maximum.  With allowed [n_allowed] column ids (device + host copy) the
 * softmax runs over those columns only (lse, logprob and argmax with it; ties to the earliest list entry) and probs [R, n_allowed]
 * receives it: whisper.decoding.detect_language's mask.  targets (device) / targets_host (host) come together; a target >= V
 * or an allowed id outside [0, V) is SSAK_ERR_INVALID.  lse, logprob, argmax, probs may each be NULL. */
int ssak_dec_embed(const void* embed_tokens, const void* embed_positions, const int32_t* ids, const int32_t* ids_host /*host*/, int B, int L,
                   int D, int V, int max_positions, int pos_offset, void* out, void* stream);
int ssak_dec_attention_fwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, int Lk, const int32_t* klens,
                           const int32_t* klens_host /*host*/, int B, int Lq, int nh, int head_dim, int causal, int q_offset, void* ctx,
                           void* stream);
int ssak_token_logprobs(const void* logits, int dtype, int R, int V, long ldv, const int32_t* targets, const int32_t* targets_host /*host*/,
                        const int32_t* allowed, const int32_t* allowed_host /*host*/, int n_allowed, float* lse, float* logprob,
                        int32_t* argmax, float* probs, void* stream);

/* ---- Whisper generation (ABI 610): single-query attention against a cache, token selection -------------------------------
 * The two kernels the greedy generation loop of ssak_amd/whisper_seq2seq.py (`generate`; ssak/infer/whisper_infer.py runs
 * model.transcribe with temperature 0 and no beam) adds to the ABI 600 entries.  NO PER-CALL HOST COPIES: neither entry takes a
 * host mirror of a device array and neither reads anything back, so the loop stays on the device between tokens.  fp32
 * accumulation in a fixed order, no float atomics: two runs on the same inputs give the same bits.
 *
 * ssak_dec_attention_step.  ctx [B, nh * 64] bf16 = softmax(q k^T * 64^-1/2 + mask) v for ONE query per (utterance, head), the
 * scaling applied to q.  q [B, ldq]; k and v are separate pointers, each with a row stride and a per-utterance stride (elements):
 * utterance b's key j is at k + b * k_batch_stride + j * ldk, head h in columns [64 h, 64 h + 64), so a cache whose capacity
 * exceeds the keys in use and the [B * S, 2 D] cross buffer are both read in place.  Key j is visible iff j < n_keys (by value:
 * the cache length of a lock-step batch) and j < klens[b]; klens [B] int32 is optional and DEVICE-ONLY: the caller that uploads
 * it validates it once (1 <= klens[b]), the kernel clamps it into [1, n_keys].  Rows that are not visible are never read.
 * The key range is cut into n_split pieces of ceil(n_keys / n_split) keys, one workgroup each; n_split = 0 lets the library choose
 * (so that the grid covers the chip at least twice where every piece keeps 128 keys; at most 16 pieces), a positive value (<= 64)
 * forces it.  With more than one piece each writes (max, sum, O[64]) in fp32 to `workspace` (16-byte aligned, at least
 * ssak_dec_attention_step_workspace_bytes(B, nh, n_split) bytes; may be NULL where one piece results) and a second kernel
 * combines them in piece order; a piece with no visible key (klens[b] ends before it starts) contributes nothing.
 * Roundings: products and sums in fp32; P is KEPT IN FP32 into the second product and the row sum is the sum of the same
 * unrounded P; ctx is rounded to bf16 once.  head_dim != 64, n_keys < 1, a stride that is not a multiple of 8 or is < nh * 64,
 * a missing or short workspace: SSAK_ERR_INVALID, nothing launched.
 *
 * ssak_dec_greedy_step.  Per row b of logits [B, ldv] fp32 (V valid columns; columns >= V are never read): the columns whose
 * byte in suppress [V] (uint8, device) is non-zero and, when first != 0, those of begin_suppress [V] count as -inf (either
 * mask may be NULL: transformers' SuppressTokensLogitsProcessor / SuppressTokensAtBeginLogitsProcessor, whisper's
 * SuppressTokens / SuppressBlank); token = the LOWEST column that attains the maximum of the processed row, logprob = its
 * log-softmax under the PROCESSED row (whisper/decoding.py: filters first, log_softmax after).  finished [B] (uint8, device) is
 * read and written: a row that was finished emits pad_id with log-prob 0 and stays finished; a row that emits eos_id becomes
 * finished.  n_unfinished [1] (int32, device) receives the number of rows still running after the step (zeroed by the entry,
 * integer atomics).  tokens[b * ldt + t] (int32) and logprobs[b * ldt + t] receive the two results; h_next [B, D] bf16 (may be
 * NULL) = bf16(fp32(embed_tokens[token]) + fp32(embed_positions[next_pos])), the next step's input row, in the same launch.
 * eos_id or pad_id outside [0, V), t outside [0, ldt), next_pos >= max_positions (with h_next): SSAK_ERR_INVALID, nothing
 * launched.  A row whose columns are ALL suppressed is the caller's error; it emits pad_id with log-prob 0. */
size_t ssak_dec_attention_step_workspace_bytes(int B, int nh, int n_split);
int ssak_dec_attention_step(const void* q, long ldq, const void* k, long ldk, long k_batch_stride, const void* v, long ldv,
                            long v_batch_stride, int n_keys, const int32_t* klens, int B, int nh, int head_dim, int n_split, void* workspace,
                            size_t workspace_bytes, void* ctx, void* stream);
int ssak_dec_greedy_step(const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                         const void* embed_tokens, const void* embed_positions, int D, int max_positions, int next_pos, int eos_id, int pad_id,
                         uint8_t* finished, int32_t* n_unfinished, int32_t* tokens, float* logprobs, long ldt, int t, void* h_next,
                         void* stream);
/* ---- Whisper timestamps (ABI 620): the token selection of a step under whisper's ApplyTimestampRules ---------------------
 * ssak_dec_timestamp_step.  ssak_dec_greedy_step -- the same outputs and conventions: tokens and log-probs at column t, finished,
 * n_unfinished, h_next, the two suppress masks and `first`, the lowest id on a tie, fixed-order sums, integer atomics only --
 * with the rules of whisper/decoding.py ApplyTimestampRules (transformers' WhisperTimeStampLogitsProcessor) applied on the
 * device, so the generation loop still reads nothing back per token.  ts_begin = the first timestamp id (no_timestamps_id + 1 in
 * Whisper's vocabularies), max_initial = the largest allowed index of the first timestamp (< 0: none), ts_last [B] int32 on the
 * device = the row's most recent sampled timestamp id or -1: at t == 0 the kernel does not read it and writes it, later it reads
 * it and updates it when it emits a timestamp (a finished row's entry is left alone).  The row's history is the n = t tokens
 * the kernel itself wrote at tokens[b * ldt + 0 .. t - 1]; of these it reads the last two.  With
 *     last = n >= 1 && tok[t - 1] >= ts_begin,   pen = n < 2 || tok[t - 2] >= ts_begin,
 * a column is allowed unless: a suppress mask hits it; it is no_timestamps_id; last && pen and it is a timestamp; last && !pen
 * and it is < eos_id; ts_last >= 0 and it lies in [ts_begin, floor) with floor = ts_last if last && !pen, else ts_last + 1;
 * n == 0 and it is < ts_begin, or > ts_begin + max_initial when max_initial >= 0.  Over the allowed columns: M = the maximum,
 * S_text / S_ts = the sums of exp(x - M) over the columns below / from ts_begin, m_text = the largest text logit.  If S_ts > 0
 * and log S_ts > m_text - M (the timestamps together outweigh every single text token) the text columns are masked as well:
 * token = the lowest timestamp arg-max, logprob = (x_token - M) - log S_ts.  Otherwise token = the lowest arg-max over all
 * allowed columns, logprob = (x_token - M) - log(S_text + S_ts).  A row with no allowed column emits pad_id with log-prob 0.
 * ts_begin <= eos_id, ts_begin >= V, no_timestamps_id outside [0, V), a NULL ts_last, and everything ssak_dec_greedy_step
 * refuses: SSAK_ERR_INVALID, nothing launched. */
int ssak_dec_timestamp_step(const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                            int ts_begin, int no_timestamps_id, int max_initial, const void* embed_tokens, const void* embed_positions, int D,
                            int max_positions, int next_pos, int eos_id, int pad_id, uint8_t* finished, int32_t* n_unfinished,
                            int32_t* tokens, float* logprobs, long ldt, int t, int32_t* ts_last, void* h_next, void* stream);
/* ---- Whisper sampling (ABI 640): the token selection of a step at temperature > 0 ------------------------------------------
 * ssak_dec_sample_step.  ssak_dec_timestamp_step's arguments, outputs and conventions, plus `temperature` and `seed`; ts_last == NULL
 * means no timestamp rules (ssak_dec_greedy_step's filters; ts_begin, no_timestamps_id and max_initial are not read).  The row is
 * filtered as those two entries filter it, the mass rule included, which fixes the candidate set: the allowed timestamp columns
 * alone when the timestamps' mass wins, else every allowed column (whisper sets logits[:, :timestamp_begin] = -inf before
 * Categorical(logits = logits / T).sample()).  token = the LOWEST column that attains the maximum of
 *     x_c * (1 / T) + g_c,   g_c = -log(-log(u_c))
 * over the set: g_c is a Gumbel variate, so the arg-max is one exact draw from softmax(x / T) over the set.  u_c depends on (seed, t,
 * row, c) through hash_u32 alone:
 *     k = hash_u32(seed, 0x5A0, (uint64(t) << 32) | row),   w = hash_u32(seed ^ (uint64(k) << 32), 0x5A1, c),
 *     u = ((w >> 9) + 0.5) * 2^-23   (strictly inside (0, 1), exact in fp32; g lies in [-2.81, 16.64]).
 * A column with x_c = -inf never wins.  logprob = (x_token - M) - log(S over the candidate set), the log-softmax of the UNTEMPERED
 * processed row.  A finished row draws nothing and emits pad_id with log-prob 0, as does a row with no allowed column.  Two calls
 * with the same arguments give the same bits.  temperature <= 0, NaN, or with a reciprocal that overflows fp32, and everything
 * ssak_dec_greedy_step refuses (with ts_last: everything ssak_dec_timestamp_step refuses): SSAK_ERR_INVALID, nothing launched. */
int ssak_dec_sample_step(const float* logits, long ldv, int B, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                         int ts_begin, int no_timestamps_id, int max_initial, const void* embed_tokens, const void* embed_positions, int D,
                         int max_positions, int next_pos, int eos_id, int pad_id, uint8_t* finished, int32_t* n_unfinished, int32_t* tokens,
                         float* logprobs, long ldt, int t, int32_t* ts_last, void* h_next, float temperature, uint64_t seed, void* stream);
/* ---- Whisper beam search (ABI 630): nb hypotheses per audio, R = B * nb rows, K = nb + 1 candidates per row ----------------
 * What whisper/decoding.py BeamSearchDecoder does per step, on the device, with the conventions of ABI 610 / 620: no host mirrors,
 * nothing read back, fp32 sums in a fixed order, integer atomics only; a refusal returns SSAK_ERR_INVALID and launches nothing.
 * 1 <= nb <= 8, B * nb <= 65535.  The rules are stated once in DESIGN.md "Whisper beam search".
 *
 * ssak_dec_beam_topk.  Per row of logits [R, ldv] fp32: the row is filtered exactly as ssak_dec_timestamp_step filters it
 * (timestamps != 0: suppress masks, `first`, ts_begin, no_timestamps_id, max_initial, the row's own history tokens[row * ldt + 0 ..
 * t - 1] and ts_last[row], the mass rule) or as ssak_dec_greedy_step does (timestamps == 0: the masks alone; tokens, ts_last and the
 * timestamp arguments are not read); logprob = the log-softmax of the processed row.  cand_token [R, K] int32 / cand_logprob [R, K]
 * fp32 receive the K largest log-probs, highest first, a tie to the lowest column; slots beyond the allowed columns hold -1 /
 * -inf.  When the mass rule fires every candidate is a timestamp.  done [B] uint8: the rows of a done audio are skipped, their
 * slots left as they are.  K must be nb + 1.
 *
 * ssak_dec_beam_select.  One step of the search per audio on cand_* and sum_logprob [B, nb] fp32 (a call starts with [0, -inf, ...]
 * per audio).  A candidate (beam j, rank r) exists when sum_logprob[j] > -inf and its token is >= 0; its score is the fp32 sum
 * sum_logprob[j] + logprob.  The candidates are walked by score descending, then j, then r: an eos_id candidate is newly finished,
 * any other becomes the next live hypothesis until nb are saved (an eos behind that point is not seen); if the candidates run out
 * the remaining live slots get sum -inf, token pad_id, source = themselves.  The newly finished are appended in walk order to the
 * audio's finished store while it holds fewer than nb: fin_tokens / fin_logprobs [B, nb, ldt] = the source's history plus eos_id
 * and its log-prob at column t, fin_len [B, nb] = t + 1, fin_sum [B, nb] = the score, n_fin [B] the count; done [B] = n_fin == nb.
 * Written in the same launch: src [R] int32 (GLOBAL row indices), tokens / logprobs [R, ldt] -- the audio's histories permuted by
 * src IN PLACE (all nb rows of t entries are read before any is written; src may repeat a source; t <= 448) and the new entries
 * at column t --, the new sums, ts_last [R] (NULL without timestamps: the new token if it is >= ts_begin, else the source's
 * value), n_unfinished [1] = the audios not done (zeroed by the entry), h_next [R, D] bf16 as ssak_dec_greedy_step forms it (may be
 * NULL).  An audio that was done on entry emits pad_id with log-prob 0, identity sources, and changes nothing else.
 *
 * ssak_dec_kv_reorder.  cache [layers, B * nb, cap, width] bf16 with element strides layer_stride / row_stride / key_stride
 * (multiples of 8, nested; 16-byte aligned base): for every layer, audio and key in [row_lo, row_hi), row r's bytes become row
 * src[r]'s, IN PLACE (a thread owns one 16-byte chunk across the audio's nb beams, loads those whose source is another beam, then
 * stores them).  Beams with src[r] == r move no bytes; bytes outside the key range and in stride gaps are untouched; a source
 * outside the audio's own beams leaves the beam as it is.  row_lo == row_hi launches nothing.  A range outside [0, cap]:
 * SSAK_ERR_INVALID.
 *
 * ssak_dec_attention_step_grouped.  ssak_dec_attention_step with `group`: query row r reads k / v of utterance r / group and
 * klens[r / group] (klens has B / group entries), so the nb beams of an audio share its cross k|v buffer.  group must divide B;
 * group = 1 is ssak_dec_attention_step, which is now this call. */
int ssak_dec_beam_topk(const float* logits, long ldv, int B, int nb, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                       int timestamps, int ts_begin, int no_timestamps_id, int max_initial, int eos_id, const int32_t* tokens, long ldt, int t,
                       const int32_t* ts_last, const uint8_t* done, int K, int32_t* cand_token, float* cand_logprob, void* stream);
int ssak_dec_beam_select(const int32_t* cand_token, const float* cand_logprob, int B, int nb, int K, int V, float* sum_logprob, int32_t* src,
                         int32_t* tokens, float* logprobs, long ldt, int t, int32_t* ts_last, int ts_begin, int32_t* fin_tokens,
                         float* fin_logprobs, int32_t* fin_len, float* fin_sum, int32_t* n_fin, uint8_t* done, int32_t* n_unfinished,
                         const void* embed_tokens, const void* embed_positions, int D, int max_positions, int next_pos, int eos_id, int pad_id,
                         void* h_next, void* stream);
int ssak_dec_kv_reorder(void* cache, const int32_t* src, int layers, int B, int nb, int cap, int width, long layer_stride, long row_stride,
                        long key_stride, int row_lo, int row_hi, void* stream);
int ssak_dec_attention_step_grouped(const void* q, long ldq, const void* k, long ldk, long k_batch_stride, const void* v, long ldv,
                                    long v_batch_stride, int n_keys, const int32_t* klens, int B, int nh, int head_dim, int n_split, int group,
                                    void* workspace, size_t workspace_bytes, void* ctx, void* stream);
/* r = res + y (either may be NULL) -> r_out (may be NULL), out = LayerNorm(r) * gamma + beta (may be NULL) on [M, C] rows of
 * dtype 0 = bf16 / 1 = fp32: the row kernel of the encoder layers without dropout sites or saved statistics.  C a multiple of
 * 8, <= 1536. */
int ssak_layernorm_fwd(const void* y, const void* res, const float* gamma, const float* beta, void* r_out, void* out, int M, int C,
                       float eps, int dtype, void* stream);

/* ---- Whisper training (ABI 650): the backward kernels of the text decoder ------------------------------------------------
 * What ssak/train/transformers/whisper_train.py:498-507,531 (the loss and loss.backward() of WhisperForConditionalGeneration)
 * needs of the decoder beyond ssak_gemm_bf16 (dgrad, wgrad with a_kmajor + accumulate, colsum, the GELU pair), ssak_cast_f32_bf16,
 * ssak_grad_sumsq(_add) and ssak_adamw_step.  Conventions of ABI 600: bf16 storage, fp32 accumulation, every sum in a fixed order,
 * NO FLOAT ATOMICS (two runs give the same bits), host copies validated before any launch (SSAK_ERR_INVALID, nothing launched),
 * head_dim 64 only.  Timing: tools/bench_whisper_train.py (DESIGN.md "Whisper fine-tuning").
 *
 * ssak_dec_attention_fwd_lse.  ssak_dec_attention_fwd plus lse [B, nh, Lq] fp32 = log sum_j exp(score_ij) over the visible keys
 * (natural log, scores scaled by 64^-1/2), NULL = not written; ssak_dec_attention_fwd is this launch with lse = NULL, its ctx
 * bit-identical.
 *
 * ssak_dec_attention_bwd.  q, k, v, klens / klens_host, causal, q_offset exactly as the forward took them; ctx and dctx
 * [B * Lq, nh * 64] bf16, lse [B, nh, Lq] as the forward wrote it.  P_ij = exp(score_ij - lse_i) on the forward's visible keys, 0
 * elsewhere; delta_i = sum_d dctx_i ctx_i (written to delta [B, nh, Lq] fp32, scratch the second kernel reads);
 * dP = dctx v^T, dS = P (dP - delta), dq = 64^-1/2 dS k, dk = 64^-1/2 dS^T q, dv = P^T dctx.  P and dS enter their products
 * rounded to bf16.  dq [B * Lq, lddq], dk [B * Lk, lddk], dv [B * Lk, lddv] bf16 with their own pointers and row strides
 * (multiples of 8, >= nh * 64; 16-byte aligned): self-attention writes the three column blocks of one packed [B * L, 3 D] buffer,
 * cross-attention dq and a [B * S, 2 D] dk|dv buffer.  Only columns [64 h, 64 h + 64) of each row are written; EVERY row is
 * written, rows of dk / dv at keys >= klens[b] as zeros.  Lq != Lk is fine (Lq 1 .. 448, Lk 1 .. 1500 are the decoder's shapes).
 *
 * ssak_dec_ce_bwd.  Per row r of fp32 logits [R, ldv] (V valid columns) with targets (device) / targets_host (host, the same
 * values; negative = HF's -100 = ignored; a target >= V is SSAK_ERR_INVALID): lse and logprob as ssak_token_logprobs defines
 * them; dlogits [R, ldd] bf16 (ldd >= V) = (exp(x_c - lse) - [c == target]) * grad_scale on a scored row, 0 on an ignored row
 * and in columns [V, ldd); row_loss [R] fp32 = -logprob (0 on an ignored row); loss_sum [1] += the sum of row_loss in a fixed
 * order (the caller zeroes it and forms HF's mean over the scored tokens).  row_loss and loss_sum may be NULL (loss_sum needs
 * row_loss): a backward whose loss the forward already has asks for dlogits alone, one launch.
 *
 * ssak_dec_embed_bwd.  dh [B * L, D] bf16, row b * L + i the gradient of ssak_dec_embed's out[b, i].  d_embed_tokens [Vp, D] fp32
 * += the rows gathered per token; d_embed_positions [max_positions, D] fp32, row pos_offset + i += sum_b dh[b, i] in batch order.
 * The gather is a CSR the caller builds from the ids it holds (ssak_amd.hip.dec_embed_csr): uniq [n_unique] the distinct ids
 * ascending, offsets [n_unique + 1] from 0 to B * L, rows [B * L] the row indices of each id ascending; device and host copies
 * of each.  One workgroup per unique id sums its rows in that order.  The host copies are validated (ids inside [0, Vp), every
 * row exactly once).
 *
 * ssak_layernorm_fwd_stats / ssak_layernorm_bwd.  The templates behind ssak_debug_layernorm_fwd / _bwd without dropout sites:
 * r = res + y -> r_out (may be NULL), out = LN(r) gamma + beta, mean / rstd [M] fp32 saved; backward: a = g1 + g2 (g2 may be
 * NULL), dr = LN_bwd(a) + g_res (g_res may be NULL), dgamma / dbeta [C] += the column sums (two-stage, fixed order);
 * workspace >= ssak_layernorm_bwd_workspace_bytes(C).  dtype 0 = bf16 / 1 = fp32; C a multiple of 8, <= 1536. */
int ssak_dec_attention_fwd_lse(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, int Lk, const int32_t* klens,
                               const int32_t* klens_host /*host*/, int B, int Lq, int nh, int head_dim, int causal, int q_offset, void* ctx,
                               float* lse, void* stream);
int ssak_dec_attention_bwd(const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, int Lk, const int32_t* klens,
                           const int32_t* klens_host /*host*/, int B, int Lq, int nh, int head_dim, int causal, int q_offset, const void* ctx,
                           const float* lse, const void* dctx, void* dq, long lddq, void* dk, long lddk, void* dv, long lddv, float* delta,
                           void* stream);
int ssak_dec_ce_bwd(const float* logits, int R, int V, long ldv, const int32_t* targets, const int32_t* targets_host /*host*/, float grad_scale,
                    void* dlogits, long ldd, float* row_loss, float* loss_sum, void* stream);
int ssak_dec_embed_bwd(const void* dh, int B, int L, int D, int Vp, int max_positions, int pos_offset, const int32_t* uniq,
                       const int32_t* offsets, const int32_t* rows, const int32_t* uniq_host /*host*/, const int32_t* offsets_host /*host*/,
                       const int32_t* rows_host /*host*/, int n_unique, float* d_embed_tokens, float* d_embed_positions, void* stream);
int ssak_layernorm_fwd_stats(const void* y, const void* res, const float* gamma, const float* beta, void* r_out, void* out, float* mean,
                             float* rstd, int M, int C, float eps, int dtype, void* stream);
size_t ssak_layernorm_bwd_workspace_bytes(int C);
int ssak_layernorm_bwd(const void* g1, const void* g2, const void* r, const float* mean, const float* rstd, const float* gamma,
                       const void* g_res, void* dr, float* dgamma, float* dbeta, int M, int C, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- Whisper LoRA (additive to ABI 660: ssak_version() is unchanged): the adapter arithmetic around a frozen nn.Linear ----
 * What peft's LoRA layer adds to the decoder's q_proj / v_proj (ssak/train/transformers/whisper_train.py:374-429; r = 32,
 * lora_alpha = 64, lora_dropout = 0.05): y += s * dropout(x) A^T B^T with s = lora_alpha / r.  x [M, D_in] bf16 with row stride
 * ldx; A [r, D_in] and B [D_out, r] contiguous (bf16 shadows of fp32 masters; ssak_lora_merge reads the masters); keep = the bits
 * of dropout site `site` under `seed` at (row, col) of x (ssak_debug_dropout_mask(seed, site, drop_p, M, D_in) reproduces them;
 * drop_p = 0: no mask), xd = keep * x / (1 - p) with the 16-bit threshold's realised p.  bf16 storage, fp32 accumulation, no
 * atomics: two calls on the same inputs give the same bits.
 *
 * Contract of the four entries: r in {8, 16, 32, 64}; D_in, D_out multiples of 64 up to 1280 (ssak_lora_merge: up to 5120, the
 * feed-forward width, for adapters merged at load); M >= 1, any remainder; row strides multiples of 8 and at least the widths;
 * operands 16-byte aligned; D_in <= 16 384 with drop_p > 0.  Anything else, or a null operand other than the ones marked optional,
 * is SSAK_ERR_INVALID before any launch.
 *
 * ssak_lora_fwd.  t [M, r] bf16 contiguous = bf16(xd A^T) (kept for the backward; NULL: not written); y[:, 0:D_out] (row stride ldy:
 * a column block of a packed q|k|v or k|v output) = bf16(float(y) + s * t B^T), in place, the product reading the rounded t.
 * ssak_lora_bwd_input.  dt [M, r] bf16 = bf16(s * dy B), dy a column block with row stride lddy; if dx is given (NULL: skipped):
 * dx = bf16((accumulate ? float(dx) : 0) + keep * (dt A) / (1 - p)), row stride lddx.
 * ssak_lora_bwd_weights.  dB [D_out, r] fp32 = s * dy^T t, dA [r, D_in] fp32 = dt^T xd (mask regenerated), both written.  The sum
 * over M: first-stage partials over fixed 512-row ranges in `workspace` (>= ssak_lora_bwd_weights_workspace_bytes), added in
 * ascending range order by a second stage.
 * ssak_lora_merge.  w_out [D_out, D_in] bf16 = bf16(w_master + s * B A): fp32 masters, fp32 FMAs in ascending r; w_out_f32 (NULL:
 * not written; may be w_master itself) receives the same value before the rounding to bf16. */
int ssak_lora_fwd(const void* x, long ldx, const void* A, const void* B, void* y, long ldy, void* t, int M, int D_in, int D_out, int r,
                  float scaling, uint64_t seed, uint32_t site, float drop_p, void* stream);
int ssak_lora_bwd_input(const void* dy, long lddy, const void* A, const void* B, void* dt, void* dx, long lddx, int accumulate, int M, int D_in,
                        int D_out, int r, float scaling, uint64_t seed, uint32_t site, float drop_p, void* stream);
size_t ssak_lora_bwd_weights_workspace_bytes(int M, int D_in, int D_out, int r);
int ssak_lora_bwd_weights(const void* dy, long lddy, const void* t, const void* dt, const void* x, long ldx, float* dB, float* dA, int M,
                          int D_in, int D_out, int r, float scaling, uint64_t seed, uint32_t site, float drop_p, void* workspace,
                          size_t workspace_bytes, void* stream);
int ssak_lora_merge(const float* w_master, const float* A, const float* B, void* w_out, float* w_out_f32, int D_in, int D_out, int r, float scaling,
                    void* stream);

/* ---- TEST-ONLY entries (not part of the product path; kept in the release library so that the parity tests run against the
 * library that ships): dropout bits of one site ------------------------------------------------------------------------
 * The engine stores no dropout mask: each site recomputes keep(seed, site, element) in its forward and backward kernels
 * (transformers draws torch's global generator at modeling_wav2vec2.py:433,458,568,571,596,692,1698; the reference passes the
 * probabilities at ssak/train/transformers/wav2vec_train.py:313-318).  These two entries write the bits out so that the CPU
 * restatement oracle/dropout_hash.py -- which feeds the SAME masks to transformers.Wav2Vec2ForCTC for the regularisers-on
 * goldens -- is pinned bit for bit against the device functions.  Since ABI 500 one definition serves every site:
 * keep(seed, site, row, col) = rowkey(seed, site, row) * colmul(col) mod 2^32 >= round(p * 65536) << 16, with (row, col) of the
 * site's row-major [rows, cols] tensor (cols <= 16 384) and, for attention, row = (b * nh + h) * F + q, col = key.  keep
 * [rows, cols] uint8; attention: keep [B, nh, F, F] (query-major).  site = the engine's stream id of the dropout site;
 * *scale_out (host, may be NULL) = the factor kept elements are multiplied by.  Never called on the hot path. */
int ssak_debug_dropout_mask(uint64_t seed, uint32_t site, float p, long rows, int cols, uint8_t* keep, float* scale_out /*host*/,
                            void* stream);
int ssak_debug_attention_dropout_mask(uint64_t seed, uint32_t site, float p, int B, int nh, int F, uint8_t* keep, void* stream);

/* ---- TEST-ONLY entries (ABI 540): the row kernels of norm_act.hip, one launch each -------------------------------------
 * Each calls the template the engine calls, instantiated for dtype 0 = bf16 (the engine) or 1 = fp32 (the fp32-exact mode);
 * activations are void* of that type, [M, C] row-major.  A dropout site is (site id, p), all sites under the launch's one
 * seed (keep bits: ssak_debug_dropout_mask on the site's [M, C] / [rows, ld] tensor); p = 0 turns a site off.
 * LayerNorm forward: r = mid(res + pre(y)) (rounded to the storage type, and stored, when r_out is given; r_out may alias y),
 * out = post(gelu?(LN(r) * gamma + beta)) with the biased variance, mean / rstd [M] fp32 (both or neither).  out = NULL is
 * the dropout-only pass (no LN: gamma, beta, mean and post must be off).  y or res may be NULL.
 * LayerNorm backward (workspace >= ssak_debug_layernorm_bwd_workspace_bytes(C)): a = post(g1 + g2) [* gelu'(xhat gamma +
 * post_gelu_beta)], dr = mid(LN_bwd(a) + g_res), dy = pre(dr) (NULL: not written); dgamma, dbeta [C] += the column sums,
 * dy_colsum [C] += those of dy (needs dy).  queued != 0 sends the second stage of the column sums through the engine's
 * deferred-reduction queue (one flush at the end of the call) instead of its own finalize launch; both sum in the same order.
 * Softmax forward: P [rows, ld] over the first min(klens[row / rows_per_batch], cols) keys (klens NULL: all cols), other
 * columns 0, a row with no valid key all 0; Pd = drop(P) (may be NULL when p = 0).  Backward: dS = P * (dP - sum(P * dP)),
 * dP = drop(dPd), columns [cols, ld) 0.  cols <= ld <= 1536, ld a multiple of 8.
 * GELU: y = gelu(x), dydx = gelu'(x) [n] fp32 as the kernels of that dtype compute them (bf16: the logistic fit of common.h;
 * fp32: erff).  Bad arguments (C not a multiple of 8 or > 1536, ld > 1536, M <= 0, p outside [0, 1), ...) are SSAK_ERR_INVALID. */
int ssak_debug_layernorm_fwd(const void* y, const void* res, const float* gamma, const float* beta, void* r_out, void* out, float* mean,
                             float* rstd, int M, int C, float eps, uint64_t seed, uint32_t pre_site, float pre_p, uint32_t mid_site,
                             float mid_p, uint32_t post_site, float post_p, int post_gelu, int dtype, void* stream);
size_t ssak_debug_layernorm_bwd_workspace_bytes(int C);
int ssak_debug_layernorm_bwd(const void* g1, const void* g2, const void* r, const float* mean, const float* rstd, const float* gamma,
                             const void* g_res, void* dr, void* dy, float* dgamma, float* dbeta, float* dy_colsum,
                             const float* post_gelu_beta, int M, int C, uint64_t seed, uint32_t pre_site, float pre_p, uint32_t mid_site,
                             float mid_p, uint32_t post_site, float post_p, int queued, int dtype, void* workspace,
                             size_t workspace_bytes, void* stream);
int ssak_debug_softmax_fwd(const void* S, void* P, void* Pd, const int32_t* klens, int rows, int cols, int ld, int rows_per_batch,
                           uint64_t seed, uint32_t site, float p, int dtype, void* stream);
int ssak_debug_softmax_bwd(const void* dPd, const void* P, void* dS, int rows, int cols, int ld, uint64_t seed, uint32_t site, float p,
                           int dtype, void* stream);
int ssak_debug_gelu(const float* x, long n, float* y, float* dydx, int dtype, void* stream);

/* ---- TEST-ONLY entry (ABI 590): the closing row kernel of an adapter layer (attn_adapter.hip), one launch -----------------
 * r2 = res + y (y may be NULL), r2' = r2 + W2 relu(W1 LN_a(r2) + b1) + b2 -> r_out (rounded to the storage type; may alias
 * res or y), out = LN_next(r2') of the stored values, mean / rstd [M] fp32 its statistics (both or neither).  LN_a = (ln_g,
 * ln_b, eps_adapter), LN_next = (next_g, next_b, eps_next), biased variance.  dtype 0: y, res, r_out, out, w1 [A,H], w2 [H,A]
 * bf16 (the products are bf16 MFMAs with fp32 accumulation, LN_a(r2) and relu(..) rounded to bf16 on the way in); dtype 1:
 * all of them fp32, fp32 FMA throughout.  A must be 16, H a multiple of 8 and <= 1536; anything else is SSAK_ERR_INVALID. */
int ssak_test_attn_adapter_fwd(const void* y, const void* res, const float* ln_g, const float* ln_b, const void* w1, const float* b1,
                               const void* w2, const float* b2, const float* next_g, const float* next_b, void* r_out, void* out,
                               float* mean, float* rstd, int M, int H, int A, float eps_adapter, float eps_next, int dtype,
                               void* stream);

/* ---- TEST-ONLY entries (ABI 550): the grouped positional convolution (posconv.hip, conv_frontend.hip), one stage each ---
 * Each calls the k_posconv_* launch functions the engine calls, with the engine's arguments (rows_per_group = K / 2 +
 * B (F + K) + K, batch stride F + K, lead = K / 2).  H hidden size, G groups, cg = H / G, K taps; activations h / dpre / out /
 * pre are [B * F, H] row-major.  dtype 0 = bf16 (the engine), 1 = fp32 (the fp32-exact mode).
 * prepare: g [K], v [H][cg][K] fp32 -> wf[o][k][c] and wb[group][c][K - 1 - k][n] (o = group * cg + n), both = g[k] v / ||v_k||
 *   in `dtype`; norms: (2 + H) K floats, [K] ||v_k||^2 first, the rest scratch.
 * pack: h -> pg [G][K / 2 + B (F + K) + K][cg] of `dtype`: K / 2 zero rows, then per utterance F frames and K zero rows, then K
 *   zero rows.
 * direct (bf16): out = [gelu](conv(h, w) + bias) for w in the wf layout (the forward: row0 = 0, pre = the pre-activation,
 *   may be NULL) or in the wb layout (the input gradient: row0 = 1 for even K, no bias / gelu / pre); pack + fragment order +
 *   posconv_direct_kernel.
 * wgrad (bf16): dwf [G][K * cg][cg] fp32 = sum over time of h[t + k - K / 2][c] dpre[t][n] (overwritten); pack of both +
 *   posconv_wgrad_kernel + posconv_wgrad_sum_kernel.
 * weight_bwd: dg [K] += , dv [H][cg][K] += the weight-norm backward of dwf; norms as left by prepare for the same g, v, of
 *   prepare's (2 + H) K floats: norms[0 .. K) is read, norms[K .. (2 + H) K) is overwritten as scratch.
 * workspace >= ssak_debug_posconv_workspace_bytes(B, F, H, G, K) (0 for a geometry the direct kernels are not built for:
 * cg = 48 or 64; K a multiple of 16 for cg = 48, of 8 for cg = 64).  Unsupported geometries are SSAK_ERR_INVALID. */
int ssak_debug_posconv_prepare(const float* g, const float* v, void* wf, void* wb, float* norms, int H, int G, int K, int dtype,
                               void* stream);
int ssak_debug_posconv_pack(const void* h, void* pg, int B, int F, int H, int G, int K, int dtype, void* stream);
size_t ssak_debug_posconv_workspace_bytes(int B, int F, int H, int G, int K);
int ssak_debug_posconv_direct(const void* h, const void* w, const float* bias, void* out, void* pre, int B, int F, int H, int G, int K,
                              int row0, int gelu, void* workspace, size_t workspace_bytes, void* stream);
int ssak_debug_posconv_wgrad(const void* h, const void* dpre, float* dwf, int B, int F, int H, int G, int K, void* workspace,
                             size_t workspace_bytes, void* stream);
int ssak_debug_posconv_weight_bwd(const float* dwf, const float* g, const float* v, float* norms, float* dg, float* dv, int H, int G,
                                  int K, void* stream);

/* ---- TEST-ONLY entries (ABI 570): the kernels that run only when the feature encoder trains (conv_frontend.hip) and the
 * data movers of the Whisper front end (whisper_frontend.hip), one k_* launch function each -----------------------------
 * dtype 0 = bf16 (the engine), 1 = fp32 (the fp32-exact mode) is the storage type of the void* activations; weights,
 * waveforms and gradients of weights are fp32.  Shapes a kernel is not built for are SSAK_ERR_INVALID before any launch.
 * conv0 = Conv1d(1, C, k = 10, s = 5): x [B, T] fp32, w [C][10], T0 = (T - 10) / 5 + 1 frames, activations [B, T0, C].
 * conv0_bwd: backward of GELU(GroupNorm_C-groups(conv0(x)) gamma + beta) from dy [B, T0, C]; sums [B][C] (mean, rstd) doubles
 *   as ssak_conv0_gn_gelu leaves them at the start of its workspace; dw [C][10], dgamma [C], dbeta [C] +=.  T >= 10, B <= 65535,
 *   C a multiple of 4, C <= 1024 and C / 4 a divisor of 256; workspace (8-byte aligned) >= ssak_debug_conv0_bwd_workspace_bytes(B, T, C).
 * conv0_wgrad: dw [C][ksize] += sum_{b,t} d[b, t, c] x[b, stride t + k], T0 = (T - ksize) / stride + 1 (ksize <= 10,
 *   64 stride + ksize <= 336, C even and <= 512); workspace >= ssak_debug_conv0_wgrad_workspace_bytes(B, C, ksize).
 * conv0_bias: out [B, T0, C] = conv0(x) + bias (bias may be NULL).  As for conv0_bwd: T >= 10, B <= 65535, C a multiple of 4,
 *   C <= 1024 and C / 4 a divisor of 256.
 * col2im: dx [B, Tin, C] = the input gradient of a channels-last Conv1d(k, s, no padding) from its column form dxcol
 *   [B, Tout, k, C]: row u sums dxcol[t][kk] over u = t s + kk; rows no window reaches are 0.  C a multiple of 8.
 * sum_slabs: out [n] = sum_b slabs[b][n], b = 0 .. nb - 1 in that order.
 * conv_weight_rearrange: out[co][kk][ci] (dtype) = w[co][ci][kk];  conv_wgrad_unrearrange: g[co][ci][kk] += dwr[co][kk][ci].
 * col2im_k3s2: out [B, RS1, H] = the input gradient of Conv1d(k = 3, s = 2, pad = 1) from dxcol [B, F, 3, H], F = (Tin + 1) / 2,
 *   times gelu'(pre); pre [B * RS1, H] holds input row u of utterance b at row b RS1 + 1 + u; rows u >= Tin of out are 0.
 *   RS1 > Tin, H a multiple of 8.
 * mel_to_cl: cl[b RS + lead + t][c] (dtype) = mel[b][c][t], mel [B, C, T] fp32; other rows of cl are left alone.
 * add_rowvec: out [B, F, H] = x + pos[t] (pos [F, H]);  copy_rows_padded: dst [B, RS, H] = src [B, F, H], rows >= F zero. */
size_t ssak_debug_conv0_bwd_workspace_bytes(int B, int T, int C);
int ssak_debug_conv0_bwd(const float* x, const float* w, const float* gamma, const float* beta, const void* dy, const double* sums,
                         float* dw, float* dgamma, float* dbeta, int B, int T, int C, int dtype, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t ssak_debug_conv0_wgrad_workspace_bytes(int B, int C, int ksize);
int ssak_debug_conv0_wgrad(const void* d, const float* x, float* dw, int B, int T, int C, int ksize, int stride, int dtype, void* workspace,
                           size_t workspace_bytes, void* stream);
int ssak_debug_conv0_bias(const float* x, const float* w, const float* bias, void* out, int B, int T, int C, int dtype, void* stream);
int ssak_debug_col2im(const void* dxcol, void* dx, int B, int Tin, int Tout, int C, int k, int s, int dtype, void* stream);
int ssak_debug_sum_slabs(const float* slabs, int nb, long n, float* out, void* stream);
int ssak_debug_conv_weight_rearrange(const float* w, void* out, int Co, int Ci, int k, int dtype, void* stream);
int ssak_debug_conv_wgrad_unrearrange(const float* dwr, float* g, int Co, int Ci, int k, void* stream);
int ssak_debug_col2im_k3s2(const void* dxcol, const void* pre, void* out, int B, int F, int Tin, int RS1, int H, int dtype, void* stream);
int ssak_debug_mel_to_cl(const float* mel, void* cl, int B, int C, int T, int RS, int lead, int dtype, void* stream);
int ssak_debug_add_rowvec(const void* x, const void* pos, void* out, int B, int F, int H, int dtype, void* stream);
int ssak_debug_copy_rows_padded(const void* src, void* dst, int B, int F, int RS, int H, int dtype, void* stream);

/* ---- TEST-ONLY entries (ABI 660): the helper kernels the wav2vec2 engine launches between its row kernels and GEMMs
 * (norm_act.hip, transpose.hip), one k_* call each; no device code of their own ------------------------------------------
 * dtype 0 = bf16 (the engine), 1 = fp32 (the fp32-exact mode) is the storage type of the void* activations.
 * specaug_fwd: h [B, F, C] in place: row (b, t) = 0 where t >= flens[b], else = embed [C] (rounded to the storage type) where
 *   mask [B, F] != 0, else untouched.  mask and flens may each be NULL (both: nothing is launched); a mask needs embed.
 * specaug_bwd: dembed [C] += the sum of the rows of dh [B, F, C] that are masked and not padding (mask and dembed given), then
 *   every masked or padding row of dh = 0.  C a multiple of 8.  scratch / scratch_floats as for colsum.
 * colsum: out [N] += sum over rows m < M of X[m * ld + n] (out is NOT zeroed first, unlike ssak_colsum_bf16); N and ld
 *   multiples of 8, ld >= N.  With rowmask [M] only rows with rowmask[m] != 0 count, and with flens too (needs rowmask and
 *   F > 0) only those with m % F < flens[m / F].  A scratch of >= min(64, ceil(M / 32)) * N floats gives the two-stage sum in
 *   a fixed order; NULL or a smaller one falls back to float atomics into out.
 * gelu_grad_mul: out = dy * gelu'(pre);  add: out = a + b (fp32 add, rounded to the storage type); n a multiple of 8.
 * transpose_batched: dst[i] [C[i]][R[i]] = src[i] [R[i]][C[i]]^T, bf16; src, dst, R, C are HOST arrays of n entries (the
 *   pointers in them device pointers).  Any shape and alignment (the 16-byte path needs R, C multiples of 8 and 16-byte-aligned
 *   pointers); more than 112 matrices are split over several launches.
 * reduce: job i is out[i][c] += sum_{k < slots[i]} partial[i][k * stride[i] + c], c < ncols[i] (HOST arrays of n entries;
 *   stride >= ncols).  The jobs are issued as ncalls consecutive k_reduce calls of call_sizes[c] jobs (1 .. 32 each, adding up
 *   to n).  use_sink != 0: the calls run under a local deferred-reduction queue (32 jobs) that is flushed once at the end; a
 *   call the queue has no room for runs at once, whole.  use_sink = 0: every call launches at once.  *queued_out / *direct_out
 *   (host, may be NULL): how many jobs went each way.  Jobs that share an out are added one after the other.
 * Bad arguments are SSAK_ERR_INVALID before any launch. */
int ssak_debug_specaug_fwd(void* h, const uint8_t* mask, const int32_t* flens, const float* embed, int B, int F, int C, int dtype,
                           void* stream);
int ssak_debug_specaug_bwd(void* dh, const uint8_t* mask, const int32_t* flens, float* dembed, int B, int F, int C, int dtype, float* scratch,
                           size_t scratch_floats, void* stream);
int ssak_debug_colsum(const void* X, long ld, int M, int N, float* out, float* scratch, size_t scratch_floats, const uint8_t* rowmask,
                      const int32_t* flens, int F, int dtype, void* stream);
int ssak_debug_gelu_grad_mul(const void* dy, const void* pre, void* out, long n, int dtype, void* stream);
int ssak_debug_add(const void* a, const void* b, void* out, long n, int dtype, void* stream);
int ssak_debug_transpose_batched(int n, const void* const* src, void* const* dst, const int* R, const int* C, void* stream);
int ssak_debug_reduce(int n, const float* const* partial, float* const* out, const long* stride, const int* slots, const int* ncols,
                      int ncalls, const int* call_sizes, int use_sink, int* queued_out, int* direct_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
