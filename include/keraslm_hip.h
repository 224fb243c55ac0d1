/* keraslm_hip.h -- C ABI of the MI355X (gfx950) Rater hot path.
 *
 * This is the drop-in boundary BELOW the reference's Python `Rater` class.  In
 * the reference the boundary is the Keras model object `Rater.model`
 * (ocrd_keraslm/lib/rating.py:56, built at rating.py:61-179); every entry point
 * here replaces one family of calls the reference makes on that object:
 *
 *   reference call site (ocrd_keraslm/lib/rating.py)        entry point here
 *   -------------------------------------------------------  -------------------
 *   Model(...) / compile, :171-178                           kl_create, kl_bind, kl_prepare
 *   model.get_weights / set_weights, :398-412, :435-458      the caller-owned flat f32 parameter vector
 *                                                            (layout: kl_param_layout) + kl_prepare
 *   model.predict_generator (windows), :516                  kl_forward_window (tgt = NULL)
 *   model.evaluate_generator, :490                           kl_forward_window (tgt != NULL)
 *   Rater.rate, :493-529, for many texts at once             kl_rate_window (one text per stream, target-only delivery)
 *   ... with the model's top-K characters and the target's rank  kl_rate_window_alts
 *   ... for a whole corpus, on the training forward (bf16)    kl_rate_window_bulk, kl_rate_scatter, kl_rate_text_bits
 *   ... with alternatives, and the suspect positions picked out  kl_rate_window_alts_bulk, kl_rate_scatter_alts, kl_rate_select
 *   ... and the suspects' alternatives rescored against what follows  kl_variant_windows (rows for kl_rate_window(_bulk))
 *   ... with a lost character inserted in front of the suspect         kl_edit_windows
 *   ... the suspect's left context read once for all its variants      kl_prefix_windows, kl_state_fanout
 *   ... for caller-supplied replacements of spans of the text          kl_span_windows, kl_span_pick
 *   ... per word: the words found, rated and the suspect ones picked out  kl_word_bounds, kl_rate_segments, kl_segment_select
 *       (the processor's mean probability per TextEquiv substring, wrapper/rate.py:308-317, for a whole corpus)
 *   ... and the suspect words' nearest entries of a lexicon, as replacements   kl_lexicon_neighbours
 *   ... or, under a table of learned confusions, its cheapest entries in a weighted distance   kl_lexicon_channel
 *   ... or, where a space was lost, the pairs of entries a run-together word falls into   kl_lexicon_splits
 *   ... or a word as a chain of up to 8 entries: compounds, more than one lost space   kl_lexicon_chains
 *   ... and the spans where a second reading of the text (another OCR engine) differs   kl_align_pairs
 *   ... and, against ground truth, the table of confusions these spans amount to   kl_confusion_counts
 *   ... and, with several such readings, their spans clustered and the readings counted   kl_witness_clusters, kl_witness_pool
 *   model.predict_on_batch, stateful (1,1) step, :566        kl_forward_window with T = 1
 *   model.predict_on_batch, incremental + states, :631       kl_step_batch
 *   ... once per character of a lattice edge, :796-851       kl_walk_batch_host (all characters of all hypotheses, one call)
 *   model.fit_generator -> train_on_batch, :292-298          kl_train_window + kl_adam_step
 *   _gen_data_from_files / _vectorize, :977-1158 (training)   kl_assemble_windows (the batches of B streams, on the device)
 *   model.reset_states, :475, :555, callbacks.py:58,69       caller zeroes its state rows
 *
 * Conventions: plain pointers and sizes only; every pointer marked "device" is
 * HBM memory owned by the CALLER (this library never allocates or frees device
 * memory and never retains a pointer beyond what kl_bind documents); every call
 * is asynchronous on the given hipStream_t (passed as void*); return value 0 =
 * success, otherwise a KL_ERR_* code (kl_error_string).  Nothing here throws.
 *
 * Data layout in HBM
 *   parameters   one flat f32 vector in Keras weight order: char embedding E [V][W],
 *                context embeddings Ctx_n [200][10], then per layer kernel K_l
 *                [D_l][4W], recurrent kernel U_l [W][4W], bias b_l [4W]; gate column
 *                order i,f,c,o (rating.py:103-145).  Gradients / Adam moments use
 *                the same layout.
 *   states       [rows][2L][W] f32, per row h1,c1,...,hL,cL (the order of
 *                Rater.predict's state lists, rating.py:622-629).  A "row" is a
 *                stateful stream (windows) or a state-pool slot (hypotheses).
 *   idx / tgt    int32 [B][T]; tgt = -1 marks an all-zero one-hot row (the padded
 *                tail of the last window, rating.py:1096-1102); ctx int32 [B][T][n_ctx].
 *   probs        f32 [B][T][V] (windows) or [n][V] (steps).
 */
#ifndef KERASLM_HIP_H
#define KERASLM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KL_ABI_VERSION 1

enum {
  KL_OK = 0,
  KL_ERR_SHAPE = 1,      /* unsupported or inconsistent dimensions */
  KL_ERR_LAUNCH = 2,     /* HIP launch / runtime error */
  KL_ERR_STATE = 3,      /* call order violated (e.g. not bound / not prepared) */
  KL_ERR_WORKSPACE = 4,  /* workspace too small */
  KL_ERR_ARG = 5         /* null or invalid argument */
  /* (negative values are never returned: the library uses them internally) */
};

/* precision of the contractions */
#define KL_PREC_BF16 1   /* bf16 MFMA operands, f32 accumulate (training)          */
#define KL_PREC_SPLIT 3  /* hi/lo split bf16 (3 MFMAs), ~f32 accuracy (rating)     */

typedef struct kl_config {
  int32_t depth;      /* L  (Rater.depth, rating.py:40)                            */
  int32_t width;      /* W  (Rater.width, rating.py:39); multiple of 32            */
  int32_t voc_size;   /* V  (Rater.voc_size, rating.py:59)                         */
  int32_t n_ctx;      /* number of context variables (1 in the reference)          */
  int32_t ctx_vocab;  /* 200 (rating.py:111)                                       */
  int32_t ctx_dim;    /* 10  (rating.py:111)                                       */
} kl_config;

typedef struct kl_handle kl_handle;

int kl_abi_version(void);
const char* kl_error_string(int code);

/* Parameter vector layout.  kl_param_layout iterates over the weight arrays in
 * Keras order; returns KL_ERR_ARG past the end. */
size_t kl_param_count(const kl_config* cfg);
int kl_param_layout(const kl_config* cfg, int index, char* name, size_t name_cap, size_t* offset, size_t* rows,
                    size_t* cols);

/* Host-only object: configuration + launch plans.  (rating.py:61-179) */
kl_handle* kl_create(const kl_config* cfg);
void kl_destroy(kl_handle* h);

/* Bind the caller's parameter vector and a scratch area for derived weights
 * (bf16 transposed copies, hi/lo splits, layer-0 look-up tables).  Both must
 * stay valid until the next kl_bind / kl_destroy. */
size_t kl_derived_bytes(const kl_handle* h);
int kl_bind(kl_handle* h, float* params /*device*/, void* derived /*device*/, size_t derived_bytes);

/* Recompute the derived weights from the bound parameters.  Call after loading
 * weights and after every parameter change made outside kl_adam_step. */
int kl_prepare(kl_handle* h, int precision, void* stream);

/* Workspace (device bytes) needed by the window calls for at most B x T. */
size_t kl_window_workspace_bytes(const kl_handle* h, int B, int T, int training);

/* Windowed forward (rating.py:490, 516, 566): B stateful streams x T steps.
 * states [B][2L][W] is read as the carried-in state and overwritten with the
 * state after step T-1.  probs (may be NULL) receives [B][T][V].  If tgt != NULL,
 * loss_acc[0] += mean categorical cross-entropy over all B*T positions and
 * loss_acc[1] += accuracy (Keras semantics, rating.py:178); loss_acc is f32[4]. */
/* Window mode of kl_forward_window / kl_train_window.  0 (default) = the reference's stateful graph:
 * a target at every position, loss and accuracy are means over all B*T positions (rating.py:161-167,
 * TimeDistributed output).  1 = its stateless graph (top LSTM layer without return_sequences,
 * rating.py:126-129, 1123-1126): one target per row, at the LAST position (tgt[b][T-1]); loss and
 * accuracy are means over the B rows, the other positions carry no gradient. */
int kl_set_window_mode(kl_handle* h, int last_only);

/* Rows the means of kl_train_window (and of kl_forward_window in bf16 precision on a training-size workspace: validation
 * windows) are taken over: 0 (default) = its B.  A caller that PADS a batch with dummy streams
 * (targets -1: no loss, no gradient) up to a stream count the persistent scans are instantiated for passes the real count
 * here, so that loss, accuracy and gradient stay those of the reference's mean over the real B*T positions
 * (rating.py:178, Keras' mean over the batch). */
int kl_set_loss_rows(kl_handle* h, int rows);

/* Ids outside their table (kl_forward_window, kl_train_window).  The caller passes 0 <= idx < voc_size and 0 <= ctx <
 * ctx_vocab; nothing here checks them, and most kernels read the row an id names.  The training forward at width 512 (the
 * second-generation wide scans, which also serve bf16 validation windows on a training-size workspace) is the exception, with
 * ONE rule on all three routes layer 0's gate inputs take there -- table offsets, gathered rows, the table of all (character,
 * context value) sums: idx is read clamped to [0, voc_size - 1], every ctx value clamped to [0, ctx_vocab - 1] (past the end:
 * the last row; negative: the first).  The sorted segment sums of kl_train_window's backward pass DROP such a position from
 * the table gradients instead, each table on its own (kl_test_segment_sums). */
int kl_forward_window(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                      float* states, float* probs, float* loss_acc, void* ws, size_t ws_bytes, void* stream);

/* Rating windows with target-only delivery (rating.py:493-529 `rate`, for many texts at once: one text per stream).
 * The recurrence and the logits are those of kl_forward_window on an inference-size workspace
 * (kl_window_workspace_bytes(.., training = 0)) in the handle's current precision, stateful window mode
 * (KL_ERR_STATE after kl_set_window_mode(h, 1)); states is advanced in the same way.  What is delivered differs:
 *   tprob  (device [B][T], or NULL)  tprob[b][t] = softmax(logits[b][t])[tgt[b][t]] where tgt >= 0 (0 is a valid target:
 *          the unmapped character), 0.0f where tgt < 0 (padded tail, dummy stream);
 *   bits   (device f64 [B], or NULL) bits[b] += sum over the positions t of stream b with tgt >= 0 of
 *          -log2(max(tprob[b][t], 1e-99)) (the clamp of rating.py:531-576), summed in f64 in a fixed order: two calls
 *          on the same inputs add bit-identical amounts;
 *   status (device f32[4], or NULL)  status[3] += 1 if a scan hand-off timed out (as loss_acc[3] of kl_forward_window).
 * No [B][T][V] array is written for the caller: 4 bytes leave the output layer per position instead of 4 V.  tgt may be
 * NULL only if tprob and bits both are (the states advance, nothing else).  ws_bytes >= kl_rate_workspace_bytes(h, B, T). */
size_t kl_rate_workspace_bytes(const kl_handle* h, int B, int T);
int kl_rate_window(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                   float* states, float* tprob, double* bits, float* status, void* ws, size_t ws_bytes, void* stream);

/* Rating windows with alternatives: kl_rate_window -- the same recurrence, logits, state advance, bits, status and error
 * returns -- delivering per position also what the model expected instead.  Within a position the V characters are
 * ordered by (logit descending, id ascending): v stands before u iff x[v] > x[u], or x[v] == x[u] and v < u (logits are
 * finite).  1 <= K <= KL_RATE_ALTS_MAX, else KL_ERR_ARG.
 *   alt_id (device int32 [B][T][K])  alt_id[b][t][j] = the j-th id in that order for j < min(K, V), -1 for j >= V;
 *   alt_p  (device f32 [B][T][K])    alt_p[b][t][j] = softmax(logits[b][t])[alt_id[b][t][j]], 0.0f where alt_id is -1;
 *   tprob  (device [B][T], or NULL)  as kl_rate_window delivers it, bit for bit;
 *   rank   (device int32 [B][T], or NULL)  the position of tgt[b][t] in the order (0: the model's first choice), -1 where
 *          tgt < 0 or tgt >= V.  Where 0 <= rank < K, alt_id[rank] == tgt and alt_p[rank] == tprob bit for bit.
 * Where tgt < 0 (padded tail, dummy stream) the position delivers nothing: tprob 0, every alt_id -1, every alt_p 0, rank -1.
 * tgt, alt_id and alt_p are required (KL_ERR_ARG); bits and status as in kl_rate_window.  8 K + 8 bytes leave the output
 * layer per position.  ws_bytes >= kl_rate_alts_workspace_bytes(h, B, T, K): the rate workspace plus a staging area for
 * the results (0 for B, T < 1 or K outside its range). */
#define KL_RATE_ALTS_MAX 8
size_t kl_rate_alts_workspace_bytes(const kl_handle* h, int B, int T, int K);
int kl_rate_window_alts(kl_handle* h, int B, int T, int K, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                        float* states, float* tprob, int32_t* alt_id, float* alt_p, int32_t* rank, double* bits,
                        float* status, void* ws, size_t ws_bytes, void* stream);

/* Bulk rating: kl_rate_window on the training forward.  Arguments, tprob / bits / status and error returns are those of
 * kl_rate_window; the recurrence, the logits and the state advance are those of kl_forward_window in KL_PREC_BF16 on a
 * training-size workspace, bit for bit (the wide persistent scans and the ring GEMM of a validation window, which take
 * thousands of streams per launch; bf16 accuracy: probabilities within 1e-2 of f64, where kl_rate_window in split
 * precision holds 2e-5).  KL_ERR_STATE unless the handle is prepared in KL_PREC_BF16, and after kl_set_window_mode(h, 1);
 * KL_ERR_WORKSPACE below kl_rate_bulk_workspace_bytes(h, B, T) = kl_window_workspace_bytes(h, B, T, 1) (0 for B, T < 1);
 * KL_ERR_ARG as in kl_rate_window; all before anything is launched.  The id rule of the training forward at width 512
 * holds here too (see kl_forward_window). */
size_t kl_rate_bulk_workspace_bytes(const kl_handle* h, int B, int T);
int kl_rate_window_bulk(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                        float* states, float* tprob, double* bits, float* status, void* ws, size_t ws_bytes, void* stream);

/* Results of rating windows in corpus order: the way back from the batches kl_assemble_windows makes.  No handle.
 * kl_rate_scatter: tprob (device f32 [B][T]) as a rating window delivered it for the batch of `plan` (the array
 *   kl_assemble_windows read: device int64 [B][4 + n_ctx], of which only start and vlen are used).  For 0 <= t < min(vlen, T)
 *   with 0 <= start + 1 + t < n_out:  out[start + 1 + t] = tprob[b][t]  -- the probability of the character tgt[b][t] was read
 *   from, at that character's position.  A bit copy; nothing else is written, a row with vlen <= 0 writes nothing.
 * kl_rate_text_bits: offsets (device int64 [n_texts + 1], ascending): text i occupies probs[offsets[i] .. offsets[i+1] - 1].
 *   bits[i] (device f64 [n_texts]) is OVERWRITTEN with -sum log2(max((double)probs[j], 1e-99)) over j = offsets[i] + 1 ..
 *   offsets[i+1] - 1 (the first character has no prediction; fewer than two characters give 0), one wave per text, summed
 *   in a fixed order: two calls on the same input give the same bits.
 * KL_ERR_ARG for null pointers, B, T or n_texts < 1, n_ctx outside 0 .. 8, misaligned pointers.  One launch each on `stream`. */
int kl_rate_scatter(const float* tprob, const int64_t* plan, int B, int T, int n_ctx, float* out, size_t n_out, void* stream);
int kl_rate_text_bits(const float* probs, const int64_t* offsets, int n_texts, double* bits, void* stream);

/* Bulk rating with alternatives: kl_rate_window_alts' delivery behind kl_rate_window_bulk's recurrence and logits.
 * Arguments, outputs (tprob, alt_id, alt_p, rank, bits, status), the order within a position and the rule for positions
 * without a target are those of kl_rate_window_alts; tgt, alt_id and alt_p are required, 1 <= K <= KL_RATE_ALTS_MAX.  tprob,
 * the state advance and bits are bit for bit those of kl_rate_window_bulk on the same inputs; where 0 <= rank < K,
 * alt_id[rank] == tgt and alt_p[rank] == tprob bit for bit.  KL_ERR_STATE unless the handle is prepared in KL_PREC_BF16, and
 * after kl_set_window_mode(h, 1); KL_ERR_WORKSPACE below kl_rate_alts_bulk_workspace_bytes(h, B, T, K) =
 * kl_rate_bulk_workspace_bytes(h, B, T) plus the staging area of the results (0 for B, T < 1 or K outside its range);
 * KL_ERR_ARG as in kl_rate_window_alts; all before anything is launched.  The id rule of the training forward at width 512
 * holds here too (see kl_forward_window). */
size_t kl_rate_alts_bulk_workspace_bytes(const kl_handle* h, int B, int T, int K);
int kl_rate_window_alts_bulk(kl_handle* h, int B, int T, int K, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                             float* states, float* tprob, int32_t* alt_id, float* alt_p, int32_t* rank, double* bits,
                             float* status, void* ws, size_t ws_bytes, void* stream);

/* kl_rate_scatter for all four results of one kl_rate_window_alts(_bulk) call.  No handle.  tprob, rank (device [B][T]) and
 * alt_id, alt_p (device [B][T][K]) as the call delivered them for the batch of `plan` (device int64 [B][4 + n_ctx]).  For
 * 0 <= t < min(vlen, T) with 0 <= g = start + 1 + t < n_out:  out_prob[g] = tprob[b][t], out_rank[g] = rank[b][t],
 * out_alt_id[g][0 .. K-1] = alt_id[b][t][0 .. K-1], out_alt_p[g][0 .. K-1] = alt_p[b][t][0 .. K-1]  (out_prob, out_rank:
 * device [n_out]; out_alt_id, out_alt_p: device [n_out][K]).  Bit copies; nothing else is written, a row with vlen <= 0
 * writes nothing.  All pointers are required.  KL_ERR_ARG for null pointers, B or T < 1, K outside 1 .. KL_RATE_ALTS_MAX,
 * n_ctx outside 0 .. 8, misaligned pointers.  One launch on `stream`. */
int kl_rate_scatter_alts(const float* tprob, const int32_t* rank, const int32_t* alt_id, const float* alt_p, const int64_t* plan,
                         int B, int T, int K, int n_ctx, float* out_prob, int32_t* out_rank, int32_t* out_alt_id,
                         float* out_alt_p, size_t n_out, void* stream);

/* Ordered selection over corpus-order results (what kl_rate_scatter_alts filled): the suspect positions.  No handle.
 * probs (device f32 [n]), rank (device int32 [n]), alt_id (device int32 [n][K]), alt_p (device f32 [n][K]).  Position j
 * (0 <= j < n) is selected iff  rank[j] >= min_rank && probs[j] <= max_prob  -- an f32 comparison, so a NaN probability is
 * never selected; min_rank >= 0 is required, so rank -1 (no prediction: a text's first character) never is either.
 *   count   (device int64 [1])  the number of selected positions, whatever `capacity` is;
 *   for i < min(count, capacity), entry i describes the i-th selected position in ascending j:
 *   sel_pos (device int64 [capacity]) = j;  sel_prob (f32 [capacity]), sel_rank (int32 [capacity]), sel_alt_id (int32
 *   [capacity][K]) and sel_alt_p (f32 [capacity][K]) are bit copies of probs[j], rank[j], alt_id[j][..], alt_p[j][..].
 * Entries from min(count, capacity) on are not written.  capacity == 0 allows null sel_* pointers: the counting call.  The
 * order does not depend on scheduling and two calls on the same input give identical output: every workgroup counts the
 * selected among its KL_RATE_SELECT_BLOCK consecutive positions, ONE workgroup of KL_RATE_SELECT_SCAN_THREADS threads turns
 * the counts into exclusive offsets (in rounds, for any number of blocks) and the total, and a third launch recomputes the
 * flags and places the records (the counting call stops after the second) -- plain launches on `stream`, no atomics, no
 * workgroup waits for another.  ws: device scratch of kl_rate_select_workspace_bytes(n) bytes (one int64 per block, 0 for
 * n < 1 or n > 2^40), 8-byte aligned.  KL_ERR_ARG for null inputs, count or ws, n < 1, K outside 1 .. KL_RATE_ALTS_MAX,
 * min_rank < 0, a NaN max_prob, null sel_* with capacity > 0, misaligned pointers; KL_ERR_WORKSPACE if ws_bytes is too
 * small; both before any launch. */
#define KL_RATE_SELECT_BLOCK 1024
#define KL_RATE_SELECT_SCAN_THREADS 256
size_t kl_rate_select_workspace_bytes(size_t n);
int kl_rate_select(const float* probs, const int32_t* rank, const int32_t* alt_id, const float* alt_p, size_t n, int K,
                   float max_prob, int min_rank, size_t capacity, int64_t* sel_pos, float* sel_prob, int32_t* sel_rank,
                   int32_t* sel_alt_id, float* sel_alt_p, int64_t* count, void* ws, size_t ws_bytes, void* stream);

/* Hypothesis windows of the selected positions (what kl_rate_select wrote): rows for kl_rate_window(_bulk) that rate the text
 * FOLLOWING a suspect under each variant of it.  No handle.  corpus (device int32 [n_corpus]) and offsets (device int64
 * [n_texts + 1], ascending, repeated values -- empty texts -- allowed) as in kl_rate_text_bits; text_ctx (device int32
 * [n_texts][n_ctx], NULL iff n_ctx == 0) the context values of every text; sel_pos (device int64 [S]) corpus positions and
 * sel_alt_id (device int32 [S][K]) their alternatives.  A suspect at g = sel_pos[s] lies in text i, offsets[i] <= g <
 * offsets[i+1] (binary search); w = corpus[g], L = min(left, g - offsets[i]), A = min(ahead, offsets[i+1] - 1 - g).  It has
 * R = K + 1 + deletions variants, row b = s * R + v:
 *   v = 0        q = x[g-L .. g-1], w, x[g+1 .. g+A]        invalid if L == 0 or g lies outside [0, min(n_corpus,
 *                                                           offsets[n_texts])) or in front of offsets[0]
 *   v = 1 .. K   the same with a = sel_alt_id[s][v-1] for w  invalid if v = 0 is, or a < 0, or a == w
 *   v = K + 1    q = x[g-L .. g-1], x[g+1 .. g+A]            (deletions == 1 only) invalid if v = 0 is, or A == 0
 * With len the length of q, a valid row is  idx[b][t] = q[t] for t < len - 1, else 0;  tgt[b][t] = q[t+1] for
 * L - 1 <= t < len - 1, else -1;  ctx[b][t][c] = text_ctx[i][c] for t < len - 1, else 0;  valid[b] = 1  -- a window from a
 * zero state over it predicts the variant's character, if it has one, and the A characters after it, and nothing else.  An
 * invalid row is a dummy stream: idx 0, ctx 0, tgt -1 everywhere, valid[b] = 0.  idx, tgt (device int32 [S*R][T]), ctx
 * (device int32 [S*R][T][n_ctx]) and valid (device int32 [S*R]) are written in every word, nothing outside them is touched;
 * a corpus position outside [0, min(n_corpus, offsets[n_texts])) reads as 0 without touching memory.  One workgroup per row,
 * one launch on `stream`, no atomics, no workgroup waits for another: the output does not depend on scheduling.
 * KL_ERR_ARG, before any launch, for null pointers (ctx and text_ctx may be null only with n_ctx == 0), S or n_texts < 1,
 * K outside 1 .. KL_RATE_ALTS_MAX, left < 1, ahead < 0, T < left + ahead or T > 1024, n_ctx outside 0 .. 8, deletions outside
 * {0, 1}, S * R > 2^22, n_corpus > 2^40, misaligned pointers (4 bytes; offsets and sel_pos 8). */
int kl_variant_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts, const int32_t* text_ctx,
                       int n_ctx, const int64_t* sel_pos, const int32_t* sel_alt_id, int S, int K, int left, int ahead,
                       int deletions, int T, int32_t* idx, int32_t* ctx, int32_t* tgt, int32_t* valid, void* stream);

/* kl_variant_windows with insertion hypotheses: for a character the text has lost in front of the suspect.  Arguments, rows,
 * outputs and launch as kl_variant_windows; with L, A, w as there, a suspect has
 *   R = K + 1 + deletions + K * insertions
 * variants, row b = s * R + v.  The rows v = 0 .. K + deletions are kl_variant_windows' rows at its indices; with
 * insertions == 1 there are K more:
 *   v = K + 1 + deletions + j  (j = 0 .. K-1)   q = x[g-L .. g-1], a, w, x[g+1 .. g+A]  with a = sel_alt_id[s][j],
 *                                               len = L + 2 + A;  invalid if v = 0 is, or a < 0
 * a == w is valid (a doubled character that lost its twin), and so is the unmapped id 0, as it is for substitution.  The rule
 * per word is kl_variant_windows': idx[b][t] = q[t] for t < len - 1, else 0;  tgt[b][t] = q[t+1] for L - 1 <= t < len - 1,
 * else -1;  ctx[b][t][c] = text_ctx[i][c] for t < len - 1, else 0;  valid[b] = 1  -- a window from a zero state over an
 * insertion row predicts a, then w, then the A characters after it.  An invalid row is the same dummy stream.  A fed row is
 * up to left + ahead + 1 long: T >= left + ahead + insertions.  insertions == 0 is kl_variant_windows, word for word.
 * KL_ERR_ARG, before any launch, for everything kl_variant_windows rejects, insertions outside {0, 1},
 * T < left + ahead + insertions, S * R > 2^22 (with this R). */
int kl_edit_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts, const int32_t* text_ctx,
                    int n_ctx, const int64_t* sel_pos, const int32_t* sel_alt_id, int S, int K, int left, int ahead, int deletions,
                    int insertions, int T, int32_t* idx, int32_t* ctx, int32_t* tgt, int32_t* valid, void* stream);

/* The left context of a suspect as a window of its own, read once for all its variants: one row per SUSPECT.  No handle.
 * corpus, offsets, text_ctx and sel_pos as in kl_variant_windows.  For suspect s < S at g = sel_pos[s] in text i (binary search,
 * as there) the row is valid iff g lies in a text, inside [0, min(n_corpus, offsets[n_texts])), and g - offsets[i] >= left: the
 * suspects whose kl_edit_windows rows have L == left.  A valid row is
 *   idx[s][t] = x[g - left + t] for t < left - 1, else 0;  ctx[s][t][c] = text_ctx[i][c] for t < left - 1, else 0;
 *   tgt[s][t] = -1 everywhere;  valid[s] = 1
 * -- a window from a zero state over it predicts nothing (it adds no bits) and leaves the state after x[g-left .. g-2].  The rows
 * of kl_edit_windows(left = 1) for the same suspect feed x[g-1] first and target from there on: continued from that state (see
 * kl_state_fanout) they compute what the rows of kl_edit_windows(left) compute from a zero state, the arithmetic cut in two.
 * An invalid row is the dummy stream: idx 0, ctx 0, tgt -1, valid[s] = 0.  idx, tgt (device int32 [S][T]), ctx (device int32
 * [S][T][n_ctx]) and valid (device int32 [S]) are written in every word, nothing outside them is touched; a corpus position
 * outside [0, min(n_corpus, offsets[n_texts])) reads as 0 without touching memory.  One workgroup per row, one launch on
 * `stream`, no atomics, no workgroup waits for another: the output does not depend on scheduling.
 * KL_ERR_ARG, before any launch, for null pointers (ctx and text_ctx may be null only with n_ctx == 0), S or n_texts < 1,
 * S > 2^22, left < 2, T < left - 1 or T > 1024, n_ctx outside 0 .. 8, n_corpus > 2^40, misaligned pointers (4 bytes; offsets
 * and sel_pos 8). */
int kl_prefix_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts, const int32_t* text_ctx,
                      int n_ctx, const int64_t* sel_pos, int S, int left, int T, int32_t* idx, int32_t* ctx, int32_t* tgt,
                      int32_t* valid, void* stream);

/* One state row handed to the rows that continue from it.  No handle.  src (device f32 [n_src][row_floats]) and dst (device
 * f32 [rows][row_floats]) are state arrays, row_floats = 2 * depth * (padded) width; parent (device int32 [rows]) names the
 * source row of every row of dst:
 *   dst[b][0 .. row_floats) = src[parent[b]][..]  for 0 <= parent[b] < n_src,  a row of zeros for any other parent[b]
 * -- a bit copy; any number of rows per parent, in any order (a fixed number R per suspect for kl_edit_windows' rows:
 * parent[b] = b / R).  Every word of dst is written, nothing else is; 16-byte loads and stores, one launch on `stream`, no
 * atomics.  KL_ERR_ARG, before the launch, for null pointers, rows or n_src < 1, row_floats not a positive multiple of 4,
 * rows * row_floats / 4 > 2^31 - 1, src or dst not 16-byte aligned (parent: 4), or dst overlapping src. */
int kl_state_fanout(const float* src, int n_src, const int32_t* parent, int rows, int row_floats, float* dst, void* stream);

/* Hypothesis windows of spans with caller-supplied replacements: the general form of kl_edit_windows, for readings that come
 * from outside the model (a second OCR engine, a lexicon, a table of confusions).  No handle.  corpus, offsets and text_ctx as
 * in kl_edit_windows.  Span s < S replaces the D = span_len[s] (device int32 [S], D >= 0; 0: an insertion in front of g)
 * written characters at corpus position g = span_start[s] (device int64 [S]) of text i = span_text[s] (device int32 [S]); it
 * owns the candidates span_first[s] .. span_first[s+1]-1 (device int64 [S + 1], ascending, span_first[0] == 0,
 * span_first[S] == C; a span may own none), and candidate c is the id string r = pool[cand_off[c] .. cand_off[c+1]-1] (pool
 * device int32 [n_pool], NULL only with n_pool == 0; cand_off device int64 [C + 1], ascending) of any length m >= 0 (0: the
 * span dropped).  Rows are numbered over all spans, N = S + C: span s has rows span_first[s] + s .. span_first[s+1] + s, the
 * first the text as written (r = w = x[g .. g+D-1]), then its candidates in order.  A call builds rows row0 .. row0 + rows - 1
 * into outputs of `rows` rows (the caller takes the row space in chunks); a row's span is found by binary search over
 * span_first[s] + s.  With n_read = min(n_corpus, offsets[n_texts]), M = max_len, L = min(left, g - offsets[i]) and
 * A = min(ahead, offsets[i+1] - g - D):
 *   span base       0 <= i < n_texts, 0 <= D <= M, offsets[i] <= g, g + D <= min(offsets[i+1], n_read), L >= 1
 *   written row     valid iff the base holds and D + A >= 1
 *   candidate row   valid iff the written row is, 0 <= m <= M, every id of r is >= 0, m + A >= 1 and r != w as id strings
 *                   (two different unmapped characters are both id 0 and count as equal); a candidate whose range does not
 *                   lie inside the pool, or whose index is not in [0, C), is invalid
 * A valid row has q = x[g-L .. g-1], r, x[g+D .. g+D+A-1], len = L + m + A, and kl_variant_windows' rule per word:
 * idx[b][t] = q[t] for t < len - 1, else 0;  tgt[b][t] = q[t+1] for L - 1 <= t < len - 1, else -1;  ctx[b][t][c] =
 * text_ctx[i][c] for t < len - 1, else 0;  valid[b] = 1  -- a window from a zero state over it predicts r and the A characters
 * after the span, and nothing else.  An invalid row is the dummy stream: idx 0, ctx 0, tgt -1, valid[b] = 0.  idx, tgt (device
 * int32 [rows][T]), ctx (device int32 [rows][T][n_ctx]) and valid (device int32 [rows]) are written in every word, nothing
 * outside them is touched; a corpus position outside [0, n_read) reads as 0 without touching memory.  One workgroup per row,
 * one launch on `stream`, no atomics, no workgroup waits for another.  With D = 1 and the candidates [a_0] .. [a_K-1], [],
 * [a_0, w] .. [a_K-1, w] the rows are kl_edit_windows(deletions = 1, insertions = 1)'s, word for word.
 * KL_ERR_ARG, before any launch, for null pointers (ctx and text_ctx may be null only with n_ctx == 0, pool only with
 * n_pool == 0), S, n_texts or rows < 1, C < 0, row0 < 0, row0 + rows > S + C, left < 1, ahead < 0, max_len outside
 * 1 .. KL_SPAN_LEN_MAX, T < left + ahead + max_len - 1 or T > 1024, n_ctx outside 0 .. 8, rows > 2^22, n_corpus, n_pool or
 * C > 2^40, misaligned pointers (4 bytes; offsets, span_start, span_first and cand_off 8). */
#define KL_SPAN_LEN_MAX 64
int kl_span_windows(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts, const int32_t* text_ctx,
                    int n_ctx, const int32_t* span_text, const int64_t* span_start, const int32_t* span_len,
                    const int64_t* span_first, int S, const int32_t* pool, size_t n_pool, const int64_t* cand_off, int64_t C,
                    int64_t row0, int rows, int left, int ahead, int max_len, int T, int32_t* idx, int32_t* ctx, int32_t* tgt,
                    int32_t* valid, void* stream);

/* The choice among every span's candidates, on the device.  cost (device f64 [S + C]) and valid (device int32 [S + C]) per row
 * of kl_span_windows' numbering (the rows' bits; what kl_span_windows said), span_first as there.  best[s] (device int32 [S])
 * is the index j within the span's candidates of the valid candidate of least cost, the smallest j among equal costs (a NaN
 * cost is never chosen); gain[s] (device f64 [S]) = cost[written] - cost[best].  best = -1 and gain = 0.0 where the written
 * row is invalid, where no candidate is valid, or where !(gain >= min_gain).  cost_out (device f64 [S + C], may be NULL, may
 * be cost itself) receives cost with +inf where the row is invalid.  One wave per span, one launch on `stream`, a fixed order
 * of reduction: two calls on the same input agree bit for bit.  KL_ERR_ARG, before the launch, for null pointers (but
 * cost_out), S < 1, C < 0 or > 2^40, misaligned pointers (valid and best 4 bytes, the others 8). */
int kl_span_pick(const double* cost, const int32_t* valid, const int64_t* span_first, int S, int64_t C, double min_gain,
                 int32_t* best, double* gain, double* cost_out, void* stream);

/* Rating under candidate contexts: every text of a corpus rated under each of C context tuples in one bulk plan (the plan rows
 * are pairs of a text and a candidate over the same ids, so kl_assemble_windows serves unchanged), the results read side by
 * side.  No handle.
 * kl_rate_scatter_planes: kl_rate_scatter with a destination plane per row.  tprob (device f32 [B][T]) and plan (device int64
 *   [B][4 + n_ctx]) as there; plane (device int32 [B]) names the candidate every row was rated under; out is device f32
 *   [C][ld] with n_out <= ld.  For 0 <= t < min(vlen, T) with 0 <= g = start + 1 + t < n_out and 0 <= plane[b] < C:
 *   out[plane[b] * ld + g] = tprob[b][t].  A bit copy; nothing else is written: a row with vlen <= 0 or a plane outside
 *   [0, C) writes nothing.  KL_ERR_ARG, before the launch, for null pointers, B, T or C < 1, C > KL_CTX_CAND_MAX, n_ctx outside
 *   0 .. 8, ld < n_out, ld > 2^40, misaligned pointers (4 bytes; plan 8).  One launch on `stream`.
 * kl_context_mix: planes (device f32 [C][ld]) as kl_rate_scatter_planes filled them; offsets (device int64 [n_texts + 1],
 *   ascending, repeated values -- empty texts -- allowed) as in kl_rate_text_bits; log2prior (device f64 [C]; NULL: uniform,
 *   every entry 0) holds finite entries or -inf (a candidate that is rated but takes no part).  For text i and its predicted
 *   positions j = max(offsets[i] + 1, 1) .. min(offsets[i+1], ld) - 1 in ascending order (the first character has no
 *   prediction; nothing outside the planes is read), all in f64:
 *     q_c[j]  = fmax((double)planes[c * ld + j], 1e-99)             (C's fmax: a NaN counts as 1e-99)
 *     lw_c(j) = log2prior[c] + sum over j' < j of log2 q_c[j']      (the candidate's weight in front of j, in bits)
 *     w_c     = exp2(lw_c(j) - max_c lw_c(j)), 0 where lw_c(j) = -inf
 *     r[j]    = sum_c w_c q_c[j] / sum_c w_c                        (the sequential Bayesian mixture of the candidates)
 *   mix[j] = (float)r[j]  (device f32 [ld], may be NULL; first characters and everything outside the texts are not written);
 *   cand_bits[i][c] = -sum_j log2 q_c[j]  (device f64 [n_texts][C]);  mix_bits[i] = -sum_j log2 r[j]  (device f64 [n_texts]);
 *   and with the final lw_c (behind the text's last character; the prior itself for a text without predictions):
 *   post[i][c] = w_c / sum_c w_c  (device f64 [n_texts][C]);  best[i] (device int32 [n_texts]) the smallest c of maximal lw_c;
 *   margin[i] (device f64 [n_texts]) = lw_best minus the largest lw_c of the others, +inf where no other is finite (C == 1).
 *   All outputs are OVERWRITTEN.  With C == 1, mix[j] is (float)q[j]: the plane bit for bit, but 0 for a NaN.  The caller
 *   guarantees one finite entry of log2prior; without one, mix, mix_bits and post are NaN, best is 0, margin +inf and
 *   cand_bits as always -- and nothing outside the outputs is touched.  One workgroup per text walks it in tiles of 64
 *   positions; every sum is taken in an order that depends on indices only, no atomics, no workgroup waits for another: two
 *   calls on the same input agree bit for bit.  Against a sequential evaluation the sums differ by rounding only.
 *   KL_ERR_ARG, before the launch, for null pointers other than mix and log2prior, n_texts < 1, C outside
 *   1 .. KL_CTX_CAND_MAX, ld < 1 or > 2^40, misaligned pointers (planes, mix and best 4 bytes, the others 8).  One launch on
 *   `stream`. */
#define KL_CTX_CAND_MAX 256
int kl_rate_scatter_planes(const float* tprob, const int64_t* plan, const int32_t* plane, int B, int T, int n_ctx, int C, float* out,
                           size_t ld, size_t n_out, void* stream);
int kl_context_mix(const float* planes, size_t ld, const int64_t* offsets, int n_texts, int C, const double* log2prior, float* mix,
                   double* cand_bits, double* mix_bits, double* post, int32_t* best, double* margin, void* stream);

/* Word-level ratings over corpus-order results (what kl_rate_scatter(_alts) filled): the words of the texts, a rating of every
 * segment, and the segments that look wrong picked out -- all on the device, in three calls.  No handle.  offsets (device int64
 * [n_texts + 1], ascending, repeated values -- empty texts -- allowed) as in kl_rate_text_bits throughout.  The two compactions
 * follow kl_rate_select: counts per KL_RATE_SELECT_BLOCK consecutive items, ONE workgroup of KL_RATE_SELECT_SCAN_THREADS threads
 * for the offsets, a third launch that places the records (the counting call stops after the second); plain launches on
 * `stream`, no atomics, no workgroup waits for another, and the output depends on indices only: two calls on the same input
 * agree bit for bit.  KL_ERR_ARG and KL_ERR_WORKSPACE are returned before anything is launched.
 *
 * kl_word_bounds: the tokeniser.  corpus (device int32 [n_corpus]) the ids, delim (device uint8 [V]) nonzero for the ids that
 *   separate words.  With lo = max(offsets[0], 0) and hi = min(n_corpus, offsets[n_texts]):
 *     is_char(j)  iff  lo <= j < hi  and not (0 <= corpus[j] < V and delim[corpus[j]] != 0)   -- an id outside the table is a
 *                                                                                                 character
 *     first(j)    iff  j == offsets[i] for some i
 *     a word starts at j      iff  is_char(j) and (first(j) or not is_char(j - 1))
 *     a word ends behind j    iff  is_char(j) and (j + 1 >= hi or first(j + 1) or not is_char(j + 1))
 *   Starts and ends alternate: the i-th start and the i-th end are one word, and a word never crosses a text boundary.
 *   count (device int64 [1]) = the number of words, whatever `capacity` is; for i < min(count, capacity), seg_start[i] and
 *   seg_end[i] (device int64 [capacity]) hold the i-th word in ascending order as [start, end).  Entries beyond are not written;
 *   capacity == 0 allows null outputs: the counting call.  Nothing outside [0, n_corpus) is read.  ws: device scratch of
 *   kl_word_bounds_workspace_bytes(n_corpus, n_texts) bytes (one int64 per block; 0 for n_corpus > 2^40 or n_texts < 1), 8-byte
 *   aligned.  KL_ERR_ARG for null corpus, offsets, delim, count or ws, null outputs with capacity > 0, n_texts < 1, V < 1,
 *   n_corpus or capacity > 2^40, misaligned pointers (corpus 4 bytes, the others but delim 8); KL_ERR_WORKSPACE if ws_bytes is too
 *   small.  n_corpus == 0 is valid: count 0.
 *
 * kl_rate_segments: probs (device f32 [n]) and rank (device int32 [n], or NULL) in corpus order; seg_start, seg_end (device
 *   int64 [S]) in any order, segments may overlap.  Segment s = [a, b) belongs to the text i with offsets[i] <= a < offsets[i+1]
 *   (binary search; empty texts are skipped); its counted positions are the j in
 *     [max(a, offsets[i] + 1), min(b, offsets[i+1], n))
 *   -- a text's first character has no prediction and is left out, and a segment ends with its text.  There are none where
 *   a < 0, b < a, a lies in no text, or a >= n.  Every output is OVERWRITTEN for every s < S:
 *     seg_n     (int32)  the number of counted positions
 *     seg_bits  (f64)    -sum log2(fmax((double)probs[j], 1e-99))            (C's fmax: a NaN counts as 1e-99)
 *     seg_psum  (f64)    sum (double)probs[j], a NaN as it is; seg_psum / seg_n is the mean probability of wrapper/rate.py:308-317
 *     seg_min   (f32)    a bit copy of the least probs[j] under `<`          (a NaN is never the minimum)
 *     seg_worst (int64)  that j, the smallest among equal values
 *     seg_bad   (int32)  how many counted j have rank[j] >= min_rank && probs[j] <= max_prob (kl_rate_select's rule, in f32);
 *                        0 with rank == NULL
 *   Where seg_n == 0, or no counted probability is below +inf (all NaN), seg_min is +inf and seg_worst -1.  A group of 16 lanes
 *   serves a segment: lane l takes the positions first + l, first + l + 16, .. in ascending order, and the 16 partial results
 *   are folded in a fixed butterfly -- the sums differ from a sequential sum by rounding only.  KL_ERR_ARG for null pointers
 *   other than rank, S < 1 or > 2^32, n_texts < 1, n > 2^40, min_rank < 0, a NaN max_prob, misaligned pointers (probs, rank,
 *   seg_n, seg_min and seg_bad 4 bytes, the others 8).  One launch.
 *
 * kl_segment_select: the records of S segments as kl_rate_segments wrote them, with seg_start and seg_end.  Segment s is
 *   selected iff  seg_n[s] >= min_n && seg_bad[s] >= min_bad && seg_bits[s] >= min_bpc * (double)seg_n[s]  (the last in f64).
 *   count (device int64 [1]) = the number selected, whatever `capacity` is; for i < min(count, capacity), in ascending s,
 *   sel_index[i] = s (device int64 [capacity]) and sel_start, sel_end, sel_n, sel_bits, sel_psum, sel_min, sel_worst, sel_bad
 *   (device [capacity], typed as the records) are bit copies of the record.  Entries beyond are not written; capacity == 0
 *   allows null sel_* pointers: the counting call.  ws: device scratch of kl_segment_select_workspace_bytes(S) bytes (0 for
 *   S < 1 or S > 2^40), 8-byte aligned.  KL_ERR_ARG for null records, count or ws, S < 1, S or capacity > 2^40, min_n < 1,
 *   min_bad < 0, min_bpc negative or NaN, null sel_* with capacity > 0, misaligned pointers (seg_n, seg_min, seg_bad and their
 *   sel_* 4 bytes, the others 8); KL_ERR_WORKSPACE if ws_bytes is too small. */
size_t kl_word_bounds_workspace_bytes(size_t n_corpus, int n_texts);
int kl_word_bounds(const int32_t* corpus, size_t n_corpus, const int64_t* offsets, int n_texts, const uint8_t* delim, int V,
                   size_t capacity, int64_t* seg_start, int64_t* seg_end, int64_t* count, void* ws, size_t ws_bytes, void* stream);
int kl_rate_segments(const float* probs, const int32_t* rank, size_t n, const int64_t* offsets, int n_texts,
                     const int64_t* seg_start, const int64_t* seg_end, size_t S, float max_prob, int min_rank, int32_t* seg_n,
                     double* seg_bits, double* seg_psum, float* seg_min, int64_t* seg_worst, int32_t* seg_bad, void* stream);
size_t kl_segment_select_workspace_bytes(size_t S);
int kl_segment_select(const int64_t* seg_start, const int64_t* seg_end, const int32_t* seg_n, const double* seg_bits,
                      const double* seg_psum, const float* seg_min, const int64_t* seg_worst, const int32_t* seg_bad, size_t S,
                      int min_n, int min_bad, double min_bpc, size_t capacity, int64_t* sel_index, int64_t* sel_start,
                      int64_t* sel_end, int32_t* sel_n, double* sel_bits, double* sel_psum, float* sel_min, int64_t* sel_worst,
                      int32_t* sel_bad, int64_t* count, void* ws, size_t ws_bytes, void* stream);

/* Lexicon look-up: the entries of a lexicon within max_dist edits of every query word -- the step between the suspect words
 * (kl_segment_select) and the replacements kl_span_windows rates.  No handle.  Words are sequences of int32 ids.
 *
 * Equality and distance.  Two ids are equal iff they are the same number AND that number lies in [0, V): an id outside the
 * range equals nothing, itself included, and never indexes a table.  lev(q, e) is the Levenshtein distance with unit costs for
 * insertion, deletion and substitution under that equality.
 *
 * The lexicon (what ratebulk.lexicon_layout_host builds): N' entries of 1 .. 64 ids, sorted by (length, original index).
 *   class_first (HOST int64 [66])  the entries of length L are the sorted positions [class_first[L], class_first[L + 1]);
 *                                  class_first[0] == class_first[1] == 0, non-decreasing, class_first[65] = N', 1 <= N' < 2^31.
 *                                  Read on the host, so that every address the kernel forms is checked before the launch.
 *   order (device int32 [N'])      the original index (>= 0) of every sorted position -- what the outputs name
 *   chars (device int32 [n_chars]) column-major within a length class: with n_L entries in class L and base[L] = sum over
 *                                  l < L of l * n_l, id j of sorted position p of class L is chars[base[L] + j * n_L +
 *                                  (p - class_first[L])]; n_chars == sum over L of L * n_L.
 * The queries: q_pool (device int32 [n_q]) and q_off (device int64 [Q + 1]); query q is q_pool[q_off[q] .. q_off[q + 1]).  A
 * query of no ids or of more than 64, and one whose offsets do not lie ascending within [0, n_q], is a neighbour of nothing, and
 * nothing of it is read.
 *
 * Every output is OVERWRITTEN for every q < Q (device int32; exact, found [Q]; cand, dist [Q][K]); nothing behind is written.
 * Over the entries e with lev(q, e) <= max_dist:
 *   exact[q]        the smallest original index with lev == 0, or -1
 *   found[q]        the number of entries with lev >= 1, whatever K is
 *   cand[q][0..K)   the original indices of the first K of these, ordered by (lev, original index); dist[q][.] their distances;
 *                   unused places are -1 in both.
 * A query that is a neighbour of nothing gets exact -1, found 0 and -1 in every place.  Duplicate entries are separate entries.
 * The statement is ratebulk.lexicon_neighbours_host.
 *
 * One workgroup per query: the query is the pattern of Myers' bit-parallel edit distance (one 64-bit word: hence the limit of
 * 64; a 32-bit word for a query of at most 32 ids unless KL_LEXICON_NARROW=0 is in the environment: same results), its match
 * masks Peq[V] lie in LDS, every lane walks whole entries of the length classes max(1, m - max_dist) ..
 * min(64, m + max_dist) and keeps its smallest keys (lev << 32 | original index) in registers; the workgroup takes the K
 * smallest in a fixed order.  Two plain launches on `stream` (the class table into ws, then the look-up), no atomics, no workgroup
 * waits for another, and the output depends on the inputs only: two calls agree bit for bit.  ws: device scratch of
 * kl_lexicon_neighbours_workspace_bytes(Q, K) bytes (the class table: the same for every Q and K), 8-byte aligned, not to be
 * shared by calls that may overlap.  KL_ERR_ARG, before any launch and with no output touched, for null pointers
 * (q_pool may be null with n_q == 0), V outside 1 .. KL_LEXICON_V_MAX, max_dist outside 0 .. KL_LEXICON_DIST_MAX, K outside
 * 1 .. KL_LEXICON_K_MAX, Q < 1 or >= 2^31, n_q or n_chars > 2^40, a class_first that breaks the rules above or disagrees with
 * n_chars, misaligned pointers (q_off, class_first and ws 8 bytes, the others 4); KL_ERR_WORKSPACE if ws_bytes is too small. */
#define KL_LEXICON_V_MAX 4096
#define KL_LEXICON_DIST_MAX 8
#define KL_LEXICON_K_MAX 16
size_t kl_lexicon_neighbours_workspace_bytes(size_t Q, int K);
int kl_lexicon_neighbours(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                          const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, int max_dist, int K, int32_t* exact,
                          int32_t* found, int32_t* cand, int32_t* dist, void* ws, size_t ws_bytes, void* stream);

/* Lexicon look-up under learned confusions: the entries of a lexicon that are cheap to reach from every query word in a
 * weighted edit distance whose steps are the plain edits and the rules of a confusion table -- the noisy-channel form of
 * kl_lexicon_neighbours.  No handle.  The lexicon (chars, n_chars, order, class_first), the queries (q_pool, n_q, q_off, Q), V
 * and the id equality are kl_lexicon_neighbours': an id outside [0, V) equals nothing, itself included.
 *
 * The channel.  rules (device int32 [R][10]) holds records in the layout kl_confusion_counts writes: src_len, tgt_len, src[4],
 * tgt[4]; rule_cost (device int32 [R]) their costs; 0 <= R <= KL_CHANNEL_RULES_MAX, both may be null with R == 0.  The SOURCE
 * is what stands in the query (the OCR word), the TARGET what stands in the entry (the truth).  unit, 1 ..
 * KL_CHANNEL_COST_MAX, is the cost of a plain insertion, deletion or substitution; max_cost, 0 .. KL_CHANNEL_COST_MAX, the
 * budget.  A rule is IGNORED, and nothing behind its used fields is read, if src_len is outside 1 .. 4, tgt_len outside
 * 0 .. 4, a used id outside [0, V) or its cost outside 0 .. KL_CHANNEL_COST_MAX (the rules lie on the device: the entry point
 * cannot refuse them).  Zero-cost rules are legal.
 *
 * Distance of a query q of m ids and an entry e of n ids: W[0][0] = 0, otherwise W[i][j] is the least of
 *   W[i-1][j-1] + (q[i-1] == e[j-1] ? 0 : unit)   (i, j > 0),     W[i-1][j] + unit   (i > 0),     W[i][j-1] + unit   (j > 0),
 *   W[i-s][j-t] + cost_r   for every rule r that is not ignored, s = src_len, t = tgt_len, i >= s, j >= t,
 *                          q[i-s:i] == src and e[j-t:j] == tgt under the id equality;
 * w(q, e) = W[m][n].
 *
 * Outputs (device int32, OVERWRITTEN for every q < Q, nothing behind them written), for a query of 1 .. 64 ids:
 *   exact[q]        the smallest original index of an entry IDENTICAL to the query (same length, all ids equal), or -1;
 *   found[q]        the number of entries that are not identical and have w <= max_cost, whatever K is;
 *   cand[q][0..K)   the original indices of the first K of these, ordered by (w, original index); cost[q][.] their w; unused
 *                   places are -1 in both.  A non-identical entry at w == 0 (zero-cost rules) is a candidate and comes first.
 * A query of no ids, of more than 64 or with bad offsets gets -1, 0 and -1 everywhere, and nothing of it is read.  With
 * R == 0 and unit == 1 the outputs are kl_lexicon_neighbours' at max_dist = max_cost.  The statement is
 * ratebulk.lexicon_channel_host.
 *
 * A preparing launch of one workgroup (the class table, the rules checked and packed, the cheapest price per id of lengthening
 * and of shortening, which bound the length classes a query can reach), then one workgroup per query: where each rule's source
 * stands in the query is settled once and kept in LDS, every lane walks whole entries with a ring of five DP columns of 16-bit
 * saturated cells in LDS (a value above max_cost is max_cost + 1), and keeps its smallest keys (w << 32 | original index); the
 * workgroup takes the K smallest in a fixed order.  Two plain launches on `stream`, no atomics on global memory, no workgroup
 * waits for another, the output depends on the inputs only: two calls agree bit for bit, and so does any order of the rules.
 * ws: device scratch of kl_lexicon_channel_workspace_bytes(Q, K, R) bytes, 8-byte aligned, not to be shared by calls that may
 * overlap.  KL_ERR_ARG, before any launch and with nothing touched, for what kl_lexicon_neighbours rejects (max_dist aside), R,
 * unit or max_cost out of range, a null rule pointer with R > 0, a misaligned rule pointer (4 bytes); KL_ERR_WORKSPACE if
 * ws_bytes is too small. */
#define KL_CHANNEL_RULES_MAX 1024
#define KL_CHANNEL_COST_MAX 4095
size_t kl_lexicon_channel_workspace_bytes(size_t Q, int K, int R);
int kl_lexicon_channel(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                       const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, const int32_t* rules,
                       const int32_t* rule_cost, int R, int unit, int max_cost, int K, int32_t* exact, int32_t* found,
                       int32_t* cand, int32_t* cost, void* ws, size_t ws_bytes, void* stream);

/* Lexicon look-up across a lost space: at which places does a query word fall into two entries of the lexicon?  The run-together
 * word (`ofthe`) beside kl_lexicon_neighbours' single entries; a spurious space (`to gether`) needs no call of its own -- the
 * joined string is an ordinary query of kl_lexicon_neighbours.  No handle.  The lexicon (chars, n_chars, order, class_first), the
 * queries (q_pool, n_q, q_off, Q), V and the id equality are kl_lexicon_neighbours': an id outside [0, V) equals nothing, itself
 * included.
 *
 * max_dist, 1 .. KL_LEXICON_DIST_MAX, is the budget of the whole split; the missing delimiter itself costs one edit, so the two
 * halves share d = max_dist - 1.  min_part, 1 .. 32, is the least number of ids of a half.  For a query q of m ids, 1 <= m <= 64,
 * and every split point s with min_part <= s <= m - min_part:
 *   best(h)   for a half h the entry minimising (lev(h, e), original index) among the entries with lev(h, e) <= d; entries at
 *             distance 0 count, duplicate entries are separate entries;
 *   s is VALID iff best(q[:s]) and best(q[s:]) both exist and total = 1 + lev_left + lev_right <= max_dist.
 * Outputs (device int32; found [Q]; split, left, right, dist [Q][K]; OVERWRITTEN for every q < Q, nothing behind them written):
 *   found[q]                       the number of valid split points, whatever K is;
 *   split, left, right, dist[q][0..K)   s, the original indices of best(q[:s]) and best(q[s:]), and total, of the first K valid
 *                                  split points ordered by (total, max(left index, right index), s) -- the nearest pair first,
 *                                  among equally near pairs the one whose rarer half is more frequent; unused places are -1 in
 *                                  all four.
 * A query with no split point (m < 2 * min_part), of no ids, of more than 64 or with bad offsets gets found 0 and -1 everywhere,
 * and nothing of the lexicon is read for it.  The statement is ratebulk.lexicon_splits_host.
 *
 * One workgroup of 256 threads per query.  Pairs of entries are never formed: after Myers' column has consumed an entry of L ids,
 * its vertical deltas hold lev(q[:i], e) for every prefix length i at once (D[i] = L + popc(Pv & low(i)) - popc(Mv & low(i))), and
 * the same walk with the reversed query over the entry read back to front holds every suffix.  Two passes over the length
 * classes max(1, min_part - d) .. min(64, m - min_part + d) (Peq[V] in LDS; the 32-bit pattern word for m <= 32 unless
 * KL_LEXICON_NARROW=0, same results) lower one key (lev << 32 | original index) per split point and side with a 64-bit unsigned
 * minimum in LDS; then thread s ranks total << 37 | max index << 6 | s among the at most 63 keys.  Two plain launches on `stream`
 * (the class table into ws, then the look-up), no atomics on global memory, no workgroup waits for another, and a minimum does
 * not depend on the order of arrival: two calls agree bit for bit.  ws: device scratch of
 * kl_lexicon_splits_workspace_bytes(Q, K) bytes (the class table), 8-byte aligned, not to be shared by calls that may overlap.
 * KL_ERR_ARG, before any launch and with nothing touched, for what kl_lexicon_neighbours rejects (max_dist 0 too) and for
 * min_part outside 1 .. 32; KL_ERR_WORKSPACE if ws_bytes is too small. */
size_t kl_lexicon_splits_workspace_bytes(size_t Q, int K);
int kl_lexicon_splits(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                      const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, int max_dist, int min_part, int K,
                      int32_t* found, int32_t* split, int32_t* left, int32_t* right, int32_t* dist, void* ws, size_t ws_bytes,
                      void* stream);

/* Lexicon chains: is a query word a concatenation of up to P exact entries of the lexicon, and of which?  The compound
 * (`arbeit|s|amt`: three entries and a linking element between two of them) and the word that lost more than one space
 * (`inthehouse`) beside kl_lexicon_splits' pairs.  No handle.  The lexicon (chars, n_chars, order, class_first), the queries
 * (q_pool, n_q, q_off, Q), V and the id equality are kl_lexicon_neighbours': an id outside [0, V) equals nothing, itself
 * included.  Duplicate entries are separate entries.
 *
 * links (HOST int32 [n_links][4]: len, ids[3]; 0 <= n_links <= KL_LEXICON_LINKS_MAX, may be null with n_links == 0) are the
 * linking elements, 1 .. KL_LEXICON_LINK_LEN_MAX ids each, every used id in [0, V); they are read on the host, as class_first
 * is.  max_parts = P, 2 .. KL_LEXICON_PARTS_MAX; min_part, 1 .. 32, the least number of ids of a piece (links do not count).
 *
 * For a query q of m ids, 1 <= m <= 64: piece(a, b), 0 <= a < b <= m and b - a >= min_part, is the smallest original index of an
 * entry identical to q[a:b], or none.  A chain of p parts is a sequence of pieces (a_1, b_1) .. (a_p, b_p) with a_1 = 0,
 * b_p = m and, between neighbours, either a_{k+1} = b_k or q[b_k:a_{k+1}] identical to one of the links; a link never stands
 * in front of the first piece or behind the last.  The key of a chain is its bottleneck, the largest piece index -- the rarest
 * part.  Per p in 1 .. P one chain of exactly p parts with the least bottleneck is reported; ties are settled by the DP, which
 * is the definition: E[1][b] = piece(0, b); for p >= 2, E[p][b] is the least of max(E[p-1][b'], piece(a, b)), the candidates
 * visited with a ascending and, per a, first b' = a (no link), then the links in index order that are identical to
 * q[a-len:a], b' = a - len >= 1; the first candidate of least key is kept (a strict <); the chain of p parts is the walk back
 * from E[p][m] through the kept predecessors.
 * Outputs (device int32; found [Q]; worst [Q][P]; entry, start, link [Q][P][P]; OVERWRITTEN for every q < Q, nothing behind
 * them written):
 *   found[q]               bit p-1 is set iff a chain of p parts exists;
 *   worst[q][p-1]          its bottleneck, or -1;
 *   entry[q][p-1][0..p)    the pieces' original indices; start[q][p-1][0..p) their a_k;
 *   link[q][p-1][0..p-1)   the index of the link between piece k and k + 1, -1 for none; unused places are -1 in all three.
 * A query of no ids, of more than 64, with bad offsets or with m < min_part gets 0 and -1 everywhere, and nothing of the lexicon
 * is read for it.  The statement is ratebulk.lexicon_chains_host.
 *
 * One workgroup of 256 threads per query.  Peq[V] of the query in LDS; a lane walks whole entries of the length classes
 * min_part .. m with a word R whose bit a says "the entry could start at a": R = low(m - L + 1), R &= Peq[c_j] >> j per entry
 * character (the 32-bit word for m <= 32 unless KL_LEXICON_NARROW=0, same results), and every bit left lowers the piece table
 * (64 x 64 words of LDS) with a 32-bit unsigned minimum.  Then thread b owns column b of the DP, one barrier per p, and thread
 * p - 1 walks back.  Two plain launches on `stream` (the class table into ws, then the look-up), no atomics on global memory,
 * no workgroup waits for another, and a minimum does not depend on the order of arrival: two calls agree bit for bit.  ws:
 * device scratch of kl_lexicon_chains_workspace_bytes(Q, P) bytes (the class table), 8-byte aligned, not to be shared by calls
 * that may overlap.  KL_ERR_ARG, before any launch and with nothing touched, for what kl_lexicon_neighbours rejects (max_dist
 * and K aside), max_parts outside 2 .. 8, min_part outside 1 .. 32, n_links outside 0 .. 8, null links with n_links > 0, a
 * link length outside 1 .. 3, a used link id outside [0, V); KL_ERR_WORKSPACE if ws_bytes is too small. */
#define KL_LEXICON_PARTS_MAX 8
#define KL_LEXICON_LINKS_MAX 8
#define KL_LEXICON_LINK_LEN_MAX 3
size_t kl_lexicon_chains_workspace_bytes(size_t Q, int P);
int kl_lexicon_chains(const int32_t* chars, size_t n_chars, const int32_t* order, const int64_t* class_first, int V,
                      const int32_t* q_pool, size_t n_q, const int64_t* q_off, size_t Q, const int32_t* links, int n_links,
                      int max_parts, int min_part, int32_t* found, int32_t* worst, int32_t* entry, int32_t* start,
                      int32_t* link, void* ws, size_t ws_bytes, void* stream);

/* Alignment of two readings: where do the texts of P pairs differ?  The step in front of kl_span_windows for a second witness of
 * the same line or page (another OCR engine): the differing spans become the spans and replacements it rates.  No handle.
 *
 * Text p of side a is a_pool[a_off[p] .. a_off[p + 1]) -- device int32 symbols [n_a] and device int64 offsets [P + 1] --, side b
 * the same.  Two symbols are equal iff they are the same number (the callers pass Unicode code points: no mapping is involved).
 *
 * Distance matrix.  With n, m the lengths of a pair: D[i][0] = i, D[0][j] = j, otherwise
 *   D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1);   d = D[n][m].
 * Status in dist[p] (device int32 [P]): d if d <= max_dist; -1 if d > max_dist -- the two are not readings of the same text;
 * |n - m| > max_dist decides that without any DP --; -2 if n > max_len or m > max_len, or if the pair's offsets are descending
 * or reach outside [0, n_a] / [0, n_b]: nothing of such a pair is read, and no address beyond max_len symbols of a pair is ever
 * formed.  For -1 and -2, n_spans[p] = 0.
 *
 * Canonical alignment.  Walk back from (n, m) and take the first of these that applies at (i, j):
 *   1. i, j > 0, a[i-1] == b[j-1] and D[i-1][j-1] == D[i][j]:  match
 *   2. i, j > 0 and D[i-1][j-1] + 1 == D[i][j]:                substitution
 *   3. i > 0 and D[i-1][j] + 1 == D[i][j]:                     deletion of a[i-1]
 *   4. otherwise:                                              insertion of b[j-1]
 *
 * Spans.  Read the operations forwards: a maximal run of non-matches is a difference; two successive differences with at most
 * `join` matches between them become one, and the matches between them belong to both sides of it.  Span s of pair p is
 * spans[(p * max_dist + s) * 4 ..] = (a_start, a_end, b_start, b_end) (device int32 [P][max_dist][4]), relative to the texts'
 * beginnings, ascending: a[a_start:a_end] reads b[b_start:b_end] in the witness.  n_spans[p] (device int32 [P]) <= d <= max_dist;
 * every place from n_spans[p] on holds -1 in all four fields, for rejected pairs too.  Two empty texts give d = 0 and no span,
 * one empty text one span.  Every output is OVERWRITTEN for every p < P; nothing behind is written.  The statement is
 * ratebulk.align_pairs_host.
 *
 * The band.  The DP runs over |i - j| <= max_dist only, which leaves all of the above unchanged for pairs with d <= max_dist: a
 * cell whose true value is at most max_dist is exact under the band, every other cell can only come out larger, and every cell
 * on an optimal path is worth at most d -- so no wrong predecessor can qualify in the walk, and D[n][m] <= max_dist under the
 * band iff it is so without.
 *
 * One workgroup of 2 * max_dist + 1 lanes (in whole waves) per pair, a grid-stride loop when P exceeds the grid of 512; the
 * anti-diagonals in turn, one barrier each, the last values in LDS; per cell the two bits of the rule that applies, in LDS while
 * (n / 16 + 1) * (2 * max_dist + 1) words fit 24 KiB, else in the workgroup's slice of ws; the walk back on one lane.  One plain
 * launch on `stream`, no atomics, no workgroup waits for another, and the output depends on the inputs only: two calls agree bit
 * for bit.  ws: device scratch of kl_align_pairs_workspace_bytes(P, max_len, max_dist) bytes (0 for arguments out of range) --
 * a slice per workgroup of the grid, not per pair, and 8 bytes where every text of max_len symbols fits LDS --, 8-byte aligned,
 * not to be shared by calls that may overlap.  KL_ERR_ARG, before any launch and with no output touched, for null pointers (a
 * pool may be null when its n_* is 0), P < 1 or >= 2^31, max_len outside 0 .. KL_ALIGN_LEN_MAX, max_dist outside
 * 1 .. KL_ALIGN_DIST_MAX, join < 0, n_a or n_b > 2^40, misaligned pointers (the offsets 8 bytes, the others 4);
 * KL_ERR_WORKSPACE if ws_bytes is too small or ws is not 8-byte aligned. */
#define KL_ALIGN_DIST_MAX 255
#define KL_ALIGN_LEN_MAX 4096
size_t kl_align_pairs_workspace_bytes(size_t P, int max_len, int max_dist);
int kl_align_pairs(const int32_t* a_pool, size_t n_a, const int64_t* a_off, const int32_t* b_pool, size_t n_b, const int64_t* b_off,
                   size_t P, int max_len, int max_dist, int join, int32_t* dist, int32_t* n_spans, int32_t* spans, void* ws,
                   size_t ws_bytes, void* stream);

/* Confusion counts: which strings of an OCR text were read as which strings of its ground truth, how often, and how often each
 * such source string stands in the OCR texts at all.  The step behind kl_align_pairs for pairs (a = OCR, b = truth); what it
 * counts is the table `keraslm-rate rescore --confusions` takes.  No handle.
 *
 * Inputs: the texts as kl_align_pairs read them (a_pool, n_a, a_off, b_pool, n_b, b_off, P, max_dist) and what it left on the
 * device (dist [P], n_spans [P], spans [P][max_dist][4]).  A pair is ACCEPTED if dist[p] >= 0 and its offsets ascend and lie
 * inside [0, n_a] / [0, n_b]; nothing of any other pair is read.  The span slots s < n_spans[p] of an accepted pair are its spans.
 *
 * Record of a span (a0, a1, b0, b1), a and b the pair's texts of n and m symbols:
 *   fields outside the texts (not 0 <= a0 <= a1 <= n and 0 <= b0 <= b1 <= m)            no record, counted as `long`
 *   a1 > a0:                          source a[a0:a1], target b[b0:b1] (an empty target: a deletion)
 *   a1 == a0 > 0:                     the OCR lost characters and a rule needs a source -- anchored on the character in front:
 *                                     source a[a0-1:a0], target b[b0-1:b1] (the run is maximal: the step before it is a match
 *                                     and both begin with the same symbol; b0 == 0, which no alignment gives, is `long`)
 *   a1 == a0 == 0, n > 0:             anchored behind: source a[0:1], target b[0:b1+1] (b1 == m is `long`)
 *   a1 == a0 == 0, n == 0:            no record, counted as `empty`
 *   more than max_chars symbols on either side after anchoring: no record, counted as `long`.
 * Symbols are equal iff they are the same number.
 *
 * Table.  The distinct records (src_len, tgt_len, src[4], tgt[4]; unused places 0) in order of first occurrence -- by pair, then
 * by span --, each with count, the number of spans that gave it, and occ, the number of positions i of the a-texts of all accepted
 * pairs with a[i:i+src_len] == source: overlapping occurrences count ("aa" stands three times in "aaaa"), none reaches across the
 * end of its text.  Records with the same source have the same occ, and count <= occ for spans of a true alignment.
 *
 * Outputs (device): rules int32 [room][10], count int64 [room], occ int64 [room] hold the first min(R, room) records, every
 * place behind them -1 in rules and 0 in count and occ; stats int64 [4] = (R: the distinct records however large room is; the
 * spans that gave a record; `long`; `empty`).  Every output is OVERWRITTEN over its whole room, nothing behind any output or
 * the workspace is written, and the outputs depend on the inputs only: two calls give the same bytes.  The statement is
 * ratebulk.confusion_counts_host.
 *
 * Eight plain launches on `stream` (confusions.hip): the records of all span slots; an open-addressing table of at least twice
 * as many slots whose entries are the least span id of a record (atomicCAS to claim, atomicMin and an integer add otherwise); the
 * ordered compaction of kl_compact.h over the spans that are their record's first; a second table of the distinct sources; a
 * walk of the accepted a-texts, one lane per position with the lengths 1 .. max_chars, that adds to the source's count; a last
 * launch that hands the counts to the records.  Integer atomics on global memory only: no sum or minimum depends on the order
 * of arrival, no lane waits for another.  ws: device scratch of kl_confusion_counts_workspace_bytes(P, max_dist, n_a) bytes (0
 * for arguments out of range), 8-byte aligned, not to be shared by calls that may overlap.  KL_ERR_ARG, before any launch and
 * with nothing touched, for null pointers (a pool may be null when its n_* is 0), P < 1 or >= 2^31, max_dist outside
 * 1 .. KL_ALIGN_DIST_MAX, max_chars outside 1 .. KL_CONFUSION_CHARS_MAX, room < 1 or > 2^40, n_a or n_b > 2^40, misaligned
 * pointers (offsets, count, occ and stats 8 bytes, the others 4); KL_ERR_WORKSPACE if ws_bytes is too small or ws is not
 * 8-byte aligned. */
#define KL_CONFUSION_CHARS_MAX 4
size_t kl_confusion_counts_workspace_bytes(size_t P, int max_dist, size_t n_a);
int kl_confusion_counts(const int32_t* a_pool, size_t n_a, const int64_t* a_off, const int32_t* b_pool, size_t n_b,
                        const int64_t* b_off, size_t P, int max_dist, const int32_t* dist, const int32_t* n_spans,
                        const int32_t* spans, int max_chars, size_t room, int32_t* rules, int64_t* count, int64_t* occ,
                        int64_t* stats, void* ws, size_t ws_bytes, void* stream);

/* Witness consensus: the differing spans of ALL witnesses of a text clustered, every witness read over a whole cluster, equal
 * readings made one and counted -- the step between kl_align_pairs and kl_span_windows, whose span and candidate arrays it leaves
 * on the device.  No handle.
 *
 * Inputs: side b as kl_align_pairs read it (b_pool, n_b, b_off, P, max_dist) and what it left on the device (dist [P], n_spans
 * [P], spans [P][max_dist][4]); pair_first (device int64 [n_texts + 1], ascending from 0 to P): text i owns the pairs
 * pair_first[i] .. pair_first[i+1]-1, its witnesses w = 0, 1, .. in that order, all aligned with that text as side a (a text
 * may own none); text_off (device int64 [n_texts + 1]): the texts' offsets in kl_span_windows' corpus, n_i = text_off[i+1] -
 * text_off[i]; join as kl_align_pairs took it.
 *
 * A text whose pair range does not lie in [0, P] in ascending order, or holds more than KL_WITNESS_MAX pairs, is counted in
 * stats[7] and nothing of it is read: pair_first lies on the device, so the entry point cannot refuse it -- a caller that wants
 * the error compares stats[7] with 0.  A pair q of any other text is ACCEPTED if dist[q] >= 0, b_off[q] <= b_off[q+1] lie inside
 * [0, n_b] (m_q their difference), 0 <= n_spans[q] <= max_dist, and every slot s < n_spans[q] has 0 <= a0 <= a1 <= n_i,
 * 0 <= b0 <= b1 <= m_q, a0 >= the previous slot's a1 and b0 >= its b1.  Every other pair is counted as `different`, and nothing
 * more of it is read.  kl_align_pairs never leaves a pair with dist >= 0 that fails the rest.
 *
 * Clusters of text i.  Take the spans (a0, a1) of its accepted pairs in order of (a0, a1, witness, slot) and sweep with a running
 * end E: a span opens a cluster iff a0 > E + join, else it joins the current one and E = max(E, a1).  The cluster is [u0, u1) =
 * [least a0, greatest a1): two differences with at most `join` equal characters between them are one -- kl_align_pairs' rule,
 * across witnesses --, spans that touch and insertions at the same place chain.
 * Reading.  The spans of witness w in a cluster are a run f .. l of its slots; without one it agrees with the text as written.
 * Else it reads b[bs:be) for text[u0:u1], bs = b0_f - (a0_f - u0), be = b1_l + (u1 - a1_l): outside its spans an alignment is
 * matches.
 * Candidates and votes.  The candidates of a cluster are its distinct readings, compared as symbols of b_pool, in order of the
 * first witness that gives one; a candidate's votes are the accepted witnesses that read it, the votes of the text as written 1
 * plus the accepted witnesses without a span in the cluster: a cluster's votes sum to 1 plus the text's accepted witnesses.
 * Dropped, and counted: `first`, a cluster with u0 == 0 (no prediction to be held against); else `long`, one with u1 - u0 >
 * KL_SPAN_LEN_MAX, a reading longer than that, or a reading range outside [0, m_q] (which no true alignment gives).
 *
 * Outputs (device), with R = P * max_dist the room -- clusters and candidates are each at most the spans there are --: the S
 * kept clusters ordered by text and u0 as kl_span_windows' spans, span_text int32 [R], span_start int64 [R] (text_off[i] + u0),
 * span_len int32 [R], span_first int64 [R + 1]; their C candidates, cand_src int64 [R] (the first position of the reading of
 * the first witness in b_pool) and cand_off int64 [R + 1] (the offsets of kl_witness_pool's pool); votes int32 [2 R] in
 * kl_span_windows' ROW numbering (row span_first[s] + s the text as written, then the span's candidates); stats int64 [8] = (S,
 * C, n_pool = cand_off[C], M: the longest kept span or reading, `different`, `first`, `long`, texts with a bad pair range).
 * Every output is OVERWRITTEN over its whole room: behind the used places -1, in votes and behind span_first[S] and cand_off[C]
 * 0.  Nothing behind an output or the workspace is written, and the outputs depend on the inputs only: two calls give the same
 * bytes.  The statement is ratebulk.witness_clusters_host.
 *
 * Four plain launches on `stream` (witnesses.hip): the fills; one WAVE per text, a lane per witness, that merges the lanes' span
 * slots by minima and maxima over the wave and settles equal readings by ballots, counting per text; kl_compact.h's one
 * workgroup that turns the counts into offsets and writes stats; the same sweep again, placing.  Integer atomics only, one per
 * wave and reason for the sums and the maximum of stats; no address outside the arrays is formed whatever bytes dist, n_spans,
 * spans or the offsets hold.  ws: device scratch of kl_witness_clusters_workspace_bytes(P, max_dist, n_texts) bytes (0 for
 * arguments out of range), 8-byte aligned, not to be shared by calls that may overlap.  KL_ERR_ARG, before any launch and with
 * nothing touched, for null pointers (b_pool may be null when n_b is 0), P or n_texts < 1 or >= 2^31, max_dist outside
 * 1 .. KL_ALIGN_DIST_MAX, join < 0, n_b > 2^40, misaligned pointers (the offsets, span_start, span_first, cand_src, cand_off
 * and stats 8 bytes, the others 4); KL_ERR_WORKSPACE if ws_bytes is too small or ws is not 8-byte aligned.
 *
 * kl_witness_pool: the candidates as ids.  pool[cand_off[c] + k] = b_ids[cand_src[c] + k] for c < C (device int32 [n_pool]; b_ids
 * device int32 [n_b], the witnesses encoded with the caller's mapping, parallel to b_pool; cand_off [C + 1] ascending from 0 to
 * n_pool, else which candidate a place is read from is undefined -- but every place of pool is written and no other).  A
 * position outside [0, n_b) reads as 0 without touching memory.  One launch, a lane per place; n_pool == 0 launches nothing.
 * KL_ERR_ARG for null pointers (b_ids with n_b == 0 and pool with n_pool == 0 may be null), C < 1, C, n_b or n_pool > 2^40,
 * misaligned pointers. */
#define KL_WITNESS_MAX 64
size_t kl_witness_clusters_workspace_bytes(size_t P, int max_dist, size_t n_texts);
int kl_witness_clusters(const int32_t* b_pool, size_t n_b, const int64_t* b_off, size_t P, int max_dist, const int32_t* dist,
                        const int32_t* n_spans, const int32_t* spans, const int64_t* pair_first, const int64_t* text_off,
                        size_t n_texts, int join, int32_t* span_text, int64_t* span_start, int32_t* span_len, int64_t* span_first,
                        int64_t* cand_src, int64_t* cand_off, int32_t* votes, int64_t* stats, void* ws, size_t ws_bytes,
                        void* stream);
int kl_witness_pool(const int32_t* b_ids, size_t n_b, const int64_t* cand_src, const int64_t* cand_off, size_t C, int32_t* pool,
                    size_t n_pool, void* stream);

/* One training batch, forward + backward (rating.py:292-298 -> train_on_batch):
 * writes the gradient of (mean CE + embedding regularisers, rating.py:187-246)
 * into grads (param layout; overwritten), advances states, and accumulates
 * loss_acc[0] CE, [1] accuracy, [2] regulariser value.  dropout_masks is NULL or
 * f32 [L][B][W] keep-masks already scaled by 1/0.9 (entry 0 unused; time-constant
 * dropout after every layer with index > 0, rating.py:146-152). */
int kl_train_window(kl_handle* h, int B, int T, const int32_t* idx, const int32_t* ctx, const int32_t* tgt,
                    float* states, const float* dropout_masks, float* grads, float* loss_acc, void* ws,
                    size_t ws_bytes, void* stream);

/* Batch assembly of stateful training (rating.py:977-1102 `_gen_data_from_files` -> `_gen_data` -> `_vectorize`, for B
 * streams at once): the caller keeps the ids of all its texts in one device vector and describes a batch by one row per
 * stream; one launch writes the three arrays kl_train_window / kl_forward_window read.
 *   corpus (device int32 [n_corpus])     the ids; a position at or beyond n_corpus reads as 0, no memory is touched there
 *   plan   (device int64 [B][4 + n_ctx]) per stream: start (position of the window's first id), vlen (how many of the T
 *          positions hold text: T, or fewer in the tail window of a text), zero_col (input column to zero, -1 = none),
 *          zero_ctx (context variable to zero, -1 = none), then the stream's n_ctx context values
 *   idx[b][t]    = t < vlen && t != zero_col ? corpus[start + t] : 0
 *   tgt[b][t]    = t < vlen ? corpus[start + t + 1] : -1
 *   ctx[b][t][c] = t < vlen && c != zero_ctx ? context value c : 0     (ctx may be NULL if n_ctx == 0)
 * (the zero-padded tail of rating.py:1096-1102 and the degraded copies of rating.py:1062-1077).  No handle: the call
 * depends on no model.  1 <= T <= 1024, 0 <= n_ctx <= 8, B >= 1; KL_ERR_ARG otherwise, and for misaligned pointers. */
int kl_assemble_windows(const int32_t* corpus, size_t n_corpus, const int64_t* plan, int B, int T, int n_ctx, int32_t* idx,
                        int32_t* ctx, int32_t* tgt, void* stream);

/* Keras-2.3 Adam with clipvalue (rating.py:178): g <- clip(g,-clip,clip);
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v updates; p -= lr_t*m/(sqrt(v)+eps); then
 * re-derives the bf16 weights (as kl_prepare).  t starts at 1. */
int kl_adam_step(kl_handle* h, const float* grads, float* m, float* v, int t, float lr, float b1, float b2,
                 float eps, float clip, void* stream);
/* The same with the gradients read as grads[i] * grad_scale (before the clip).  Data-parallel training (not a
 * reference feature: rating.py:295 trains with workers=1) all-reduces the flat gradient vector with SUM and passes
 * 1 / world size here, so the mean over the ranks costs no pass of its own. */
int kl_adam_step_scaled(kl_handle* h, const float* grads, float grad_scale, float* m, float* v, int t, float lr,
                        float b1, float b2, float eps, float clip, void* stream);

/* Incremental step for n hypotheses with explicit states (rating.py:578-639):
 * row i reads its state from pool slot slot_in[i] and writes the new state to
 * slot_out[i] (slot_out must not alias any slot_in of the same call); probs
 * receives [n][V].  pool is [n_slots][2L][W] f32.  ctx is [n][n_ctx]. */
size_t kl_step_workspace_bytes(const kl_handle* h, int n);
int kl_step_batch(kl_handle* h, int n, const int32_t* idx, const int32_t* ctx, float* pool, const int32_t* slot_in,
                  const int32_t* slot_out, float* probs, void* ws, size_t ws_bytes, void* stream);

/* The same step as a BEAM SEARCH issues it (rating.py:809-826 rate_best, :689-691 generate, each through
 * Rater.predict, rating.py:578-639): one call per character with the GPU idle in between, so what counts is the time
 * from the call to the numbers being in the caller's hands, not the kernels' own.  Differences to kl_step_batch:
 *   - idx, ctx, slot_in, slot_out (and target) are HOST arrays; up to 256 hypotheses they travel inside the kernel
 *     arguments of the launches (no copy to the device, no index array for the kernels to chase), beyond that in one copy;
 *   - the results are delivered into HOST memory the device can write (kl_host_alloc): probs_host receives [n][V], or --
 *     target != NULL -- [n]: per row the probability of character target[i] alone (all a lattice decoder looks at,
 *     rating.py:838-843); head_k > 0 also delivers the first head_k state vectors of every new state, [n][head_k][W]
 *     (history clustering compares exactly those, rating.py:887-916);
 *   - nothing has to synchronise with the stream: *done_host becomes `ticket` once everything above has arrived
 *     (kl_step_wait spins on that word; use a different ticket for every step).
 * pool, ws: device.  ws_bytes >= kl_step_host_workspace_bytes(h, n); one workspace per handle and stream. */
void* kl_host_alloc(size_t bytes);      /* zeroed, page-locked, device-visible host memory; NULL on failure */
void kl_host_free(void* p);
size_t kl_step_host_workspace_bytes(const kl_handle* h, int n);
int kl_step_batch_host(kl_handle* h, int n, const int32_t* idx, const int32_t* ctx, const int32_t* slot_in,
                       const int32_t* slot_out, const int32_t* target, float* pool, int head_k, float* probs_host,
                       float* heads_host, uint32_t* done_host, uint32_t ticket, void* ws, size_t ws_bytes, void* stream);
/* A LATTICE EDGE in one call (rating.py:796-851 rate_best: every hypothesis walks through the fixed text of its
 * alternative, so all characters it will feed are known before the first step).  Row i takes len[i] steps
 * (1 <= len[i] <= 1024); idx, target, slot_step and tprob_host are RAGGED: row i occupies entries off[i] .. off[i] + len[i] - 1,
 * off = prefix sum of len, total = sum of len.  ctx is [n][n_ctx].  All index arrays are HOST arrays.
 * Semantics: exactly those of len[i] chained kl_step_batch calls on row i --
 *   step t feeds idx[off + t] into the state step t - 1 left (t = 0: pool slot slot_in[i]) and writes the new state to pool
 *   slot slot_step[off + t]; tprob_host[off + t] = softmax probability of character target[off + t] after that step (0 is a
 *   valid target; a target outside 0 .. V - 1 delivers 0.0f); the last slot_step entry of a row holds its final state;
 *   head_k > 0 also delivers the first head_k state vectors of every row's FINAL state, [n][head_k][W], as
 *   kl_step_batch_host does.
 * No slot_step entry may equal a slot_in of the call or another slot_step entry; slots named in slot_in are never written.
 * Rows may come in any order (the library orders them so that the rows still active at a step form a prefix), n may be any
 * positive count (more than 256 rows are walked in groups inside the call).
 * Launches: per step only the cell kernels, indices in the kernel arguments (the conditions of kl_step_batch_host's
 * 256-hypothesis path: one context variable, widths 64, 128 or a multiple of 256, V <= 65535, ctx_vocab <= 65536;
 * KL_HOST_KERNARG=0 disables it); everything else chains kl_step_batch on ONE staged upload of all indices.  The output
 * layer is deferred in both:
 * after the last step one launch contracts the top layer's h of all `total` (row, step) pairs with the embedding, keeps
 * a running maximum and sum per pair and delivers 4 bytes per pair -- no [total][V] array exists.  That launch serves EVERY
 * vocabulary and width the library accepts (any V, W % 32 == 0): there is no logits-GEMM fall-back.
 * tprob_host, heads_host, done_host, stage_host: from kl_host_alloc; stage_host >= kl_walk_stage_bytes(h, n, total) bytes:
 * every index that does not travel in kernel arguments is copied there before the call returns, so the caller's (pageable)
 * arrays are not read afterwards.  *done_host becomes `ticket` once everything has arrived (kl_step_wait); until then
 * stage_host and the result buffers belong to the call.  ws: device, >= kl_walk_workspace_bytes(h, n, total), one per
 * handle and stream.  KL_ERR_ARG (null pointer, n < 1, a len outside 1 .. 1024, head_k out of range), KL_ERR_STATE (not
 * prepared) and KL_ERR_WORKSPACE are returned before anything is launched. */
size_t kl_walk_workspace_bytes(const kl_handle* h, int n, int total);   /* total = sum of len[i] */
size_t kl_walk_stage_bytes(const kl_handle* h, int n, int total);
int kl_walk_batch_host(kl_handle* h, int n, const int32_t* len, const int32_t* idx, const int32_t* target,
                       const int32_t* ctx, const int32_t* slot_in, const int32_t* slot_step, float* pool, int head_k,
                       float* tprob_host, float* heads_host, void* stage_host, uint32_t* done_host, uint32_t ticket,
                       void* ws, size_t ws_bytes, void* stream);
/* returns 0 once *done_host == ticket; KL_ERR_LAUNCH / KL_ERR_STATE after timeout_s seconds without it */
int kl_step_wait(const uint32_t* done_host, uint32_t ticket, double timeout_s);

/* One expansion and pruning step of generate's beam search ON THE DEVICE (rating.py:689-707: per hypothesis the 10 most
 * likely characters with p >= 0.004, every continuation insorted by running cost, the first 256 kept), for `rows`
 * hypotheses (1 .. 256) fanning out to at most `fan` (1 .. 16) continuations each.  All pointers are DEVICE pointers.
 *   probs [rows][V] f32     what kl_step_batch just wrote (V = the handle's voc_size; 0 <= p <= 1)
 *   cum_in [rows] f32       running cost per row, +inf = dead row (no candidates)
 *   slot_new [rows]         the pool slots that step wrote (a survivor's next slot_in is its parent's entry)
 *   valid [V] bytes         non-zero = the id may be generated; NULL = every id except 0
 *   floor                   pass 0.004f (p >= floor is compared in f32; equal to the reference's f64 comparison for every f32 p)
 * The reference's bookkeeping as a total order:
 *   candidates of a live row = its `fan` largest probabilities -- equal values by smaller id first (this library's
 *     definition: the reference leaves such ties to an unstable sort) --, of those the ones with p >= floor, of those the valid
 *     ids (an invalid id among the `fan` largest still occupies its place);
 *   cum = cum_in[row] + (-logf(p)): accurate logf, one f32 addition;
 *   insertion sequence = row * fan + k, k counting a row's candidates from the least to the most probable;
 *   survivors = the first `rows` candidates by (cum ascending, insertion sequence DESCENDING) -- what insort_left (a later
 *     equal key goes in front) and truncation after every insertion leave.
 * Outputs, entry i = survivor i in that order: idx_next (character id), slot_in_next (= slot_new[parent]), cum_next for the
 * next step; parent_log (row index in THIS step), idx_log, cum_log for the log (a *_log pointer may equal its *_next
 * pointer).  Entries beyond the survivors: id 0, zero_slot, +inf, parent -1.  *n_live = number of survivors.
 * ws: device, >= kl_beam_workspace_bytes(h, rows, fan) (0 for arguments out of range), one per handle and stream.
 * KL_ERR_ARG (null pointer, rows outside 1 .. 256, fan outside 1 .. 16) and KL_ERR_WORKSPACE are returned before anything is
 * launched.  Two launches on `stream`, no synchronisation, no host memory touched. */
size_t kl_beam_workspace_bytes(const kl_handle* h, int rows, int fan);
int kl_beam_expand(kl_handle* h, int rows, int fan, float floor, const float* probs, const uint8_t* valid,
                   const float* cum_in, const int32_t* slot_new, int32_t zero_slot, int32_t* idx_next,
                   int32_t* slot_in_next, float* cum_next, int32_t* parent_log, int32_t* idx_log, float* cum_log,
                   int32_t* n_live, void* ws, size_t ws_bytes, void* stream);

/* One DRAWN character per row ON THE DEVICE, for sampling continuations (Rater.sample): `rows` independent chains (1 .. 1024)
 * advance in lockstep, each continuing from the state it just wrote, so a step is kl_step_batch followed by this call and the
 * host waits once per text, not once per character.  All pointers are DEVICE pointers.
 *   probs [rows][V] f32     what kl_step_batch just wrote (V = the handle's voc_size)
 *   valid [V] bytes         non-zero = the id may be drawn; NULL = every id except 0 (as in kl_beam_expand)
 *   temperature             >= 0 and finite; 0 = greedy
 *   top_k                   0 .. 64, 0 = off;  floor >= 0
 *   seed, step              the random stream and the position in it (one step per character)
 *   cum_in, cum_next [rows] running cost per chain before and after (they may be the same array)
 *   idx_next [rows] int32   the drawn id;  u_log [rows] f32, may be NULL: the uniform number the row drew with
 * Per row r:
 *   Uniform number.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with key
 *     (seed & 0xffffffff, seed >> 32) and counter (step, r, 0, 0); of the first output word x0, u = (x0 >> 8) * 2^-24, in
 *     [0, 1).  Integer arithmetic only: lib/gensample.py philox_uniform gives the same bits.  u is computed (and logged) at
 *     every temperature, 0 included.
 *   Candidates.  The valid ids; if top_k > 0, the first min(top_k, valid ids) of them in the order (p descending, id
 *     ascending) -- kl_rate_window_alts' total order, taken over the valid ids only --; of those the ids with p >= floor (an
 *     f32 comparison).  If that leaves none, the single candidate is the first valid id of that order.  If no id is valid,
 *     the pick is id 0 at cost +inf.
 *   Pick, temperature == 0: the first candidate of that order.
 *   Pick otherwise: weight w_v = p_v at temperature 1, else expf((logf(p_v) - logf(p_max)) / temperature), p_max the largest
 *     candidate probability; p_v == 0 gives weight 0.  S = the sum of the weights.  The pick is the smallest candidate id
 *     whose running weight sum exceeds u * S, running sums taken in ID-ASCENDING order; if rounding leaves none, the last
 *     candidate of positive weight.  A candidate of weight 0 is never picked (if every candidate's probability is 0, the pick is
 *     the first candidate, at cost +inf).  The order of the additions is fixed: two calls on the same inputs pick bit-identically.
 *   Cost.  cum_next[r] = cum_in[r] + (-logf(p_pick)): accurate logf, one f32 addition, as kl_beam_expand does it.
 * kl_sample_pick_from is the same call with counter (step, row0 + r, 0, 0) (modulo 2^32): more than 1024 chains are drawn in
 * groups of rows that continue each other's row numbers, so no two chains share a random number.
 * ws: device, >= kl_sample_workspace_bytes(h, rows) (0 for rows out of range), one per handle and stream (vocabularies above
 * 256 keep a row's weights there between summing them and picking; smaller ones do not touch it).
 * KL_ERR_ARG (null probs / cum_in / idx_next / cum_next, rows outside 1 .. 1024, top_k outside 0 .. 64, temperature negative,
 * NaN or infinite, floor negative or NaN) and KL_ERR_WORKSPACE are returned before anything is launched.  One launch on
 * `stream`, no synchronisation, no host memory touched. */
size_t kl_sample_workspace_bytes(const kl_handle* h, int rows);
int kl_sample_pick(kl_handle* h, int rows, const float* probs, const uint8_t* valid, float temperature, int top_k,
                   float floor, uint64_t seed, uint32_t step, const float* cum_in, int32_t* idx_next, float* cum_next,
                   float* u_log, void* ws, size_t ws_bytes, void* stream);
int kl_sample_pick_from(kl_handle* h, int rows, uint32_t row0, const float* probs, const uint8_t* valid, float temperature,
                        int top_k, float floor, uint64_t seed, uint32_t step, const float* cum_in, int32_t* idx_next,
                        float* cum_next, float* u_log, void* ws, size_t ws_bytes, void* stream);

/* THE BEAM BOOKKEEPING OF MANY LATTICE EDGES ON THE DEVICE (rating.py:796-851, Rater.rate_best_batch): after one
 * kl_walk_batch_host over the hypotheses of E edges, two launches turn its probabilities into every edge's new beam.  The
 * statement both implement is lib/lattice_batch.py (edge_costs_host, edge_decode_host): results agree with it bit for bit.
 * Both: caller's stream, no device memory owned, no host synchronisation, nothing launched when a code is returned; two calls
 * on the same inputs are bit-identical.  All pointers are DEVICE pointers (probs may be device-visible host memory).
 *
 * kl_edge_costs: cost[s] = -(log(max((double)probs[s], 1e-99)) / log(2.0)) * lm_weight + alt_conf[pair_alt[s]] for the n_pairs
 *   (track, step) pairs, every operation an IEEE f64 operation of its own (what the host computes with math.log(p, 2); the
 *   device's log is within 1 ulp of the host's).  probs may be the walk's kl_host_alloc result buffer: launched on the walk's
 *   stream it reads what the walk delivered, without a host wait in between.  KL_ERR_ARG: null or misaligned pointers, n_pairs
 *   outside 1 .. 2^40, a NaN lm_weight.
 *
 * kl_edge_decode: E edges, one workgroup of one wave each.
 *   desc [E][8] int32       n_in, n_alt, n_pre, in_off, alt_off, trk_off, pre_off, max_batches -- counts and offsets into:
 *   cum_in f64              per incoming hypothesis: cumulative cost
 *   alt_len, alt_class      per alternative: characters, text-class id (equal texts share one)
 *   step_off, final_slot    per track (hypothesis-major, alternative-minor; track t of an edge = hypothesis t / n_alt,
 *                           alternative t % n_alt): offset of its step costs in `cost`, slot of its state after the last step
 *                           (a track of an empty alternative has no steps: final_slot holds its hypothesis' slot)
 *   pre_cost f64, pre_class, pre_slot   per entry other in-edges already left at the destination, in beam order (may be
 *                           null if no edge has any)
 *   cost f64                per (track, step) pair (kl_edge_costs)
 *   pool, depth_k, dist     history clustering: depth_k = 0 off; else two entries of one class are close when for each of
 *                           the first depth_k state vectors the squared distance of their slots (kl_state_dist2's sum) is
 *                           < dist * dist
 *   batch_size, beam_width  as Rater.batch_size and rate_best's beam_width
 *   cap_tracks              1 .. 1024: tracks per edge the launch reserves LDS for (46 bytes each + 768)
 *   out                     one block of kl_edge_decode_out_bytes(E, beam_width, n_tracks, n_pairs) bytes, parts 8-byte aligned:
 *                           cost f64 [E][beam_width] | count int32 [E] | status [E] | ref [E][beam_width] | consumed
 *                           [n_tracks] | when [n_pairs].  Per edge: count = survivors (<= beam_width), ref = track number or
 *                           -1 - j for the j-th pre-existing entry, cost = its cumulative cost (entries beyond count: 0);
 *                           consumed = characters every track took; when[step_off + k] = batch number * 1024 + place in
 *                           the batch at which a track took its k-th step (defined for the steps taken).
 *   status 1: the edge was not decoded (n_in * n_alt > cap_tracks, n_pre > 64, an alternative above 65535 characters,
 *   max_batches outside 1 .. 2^20, negative counts, a NaN cost); count is 0, its other outputs are undefined, other edges are
 *   not affected.  KL_ERR_ARG: null or misaligned pointers, E, batch_size, beam_width < 1, cap_tracks outside 1 .. 1024,
 *   depth_k outside 0 .. 2 * depth, depth_k > 0 without pool or with a NaN dist; KL_ERR_WORKSPACE: out_bytes too small. */
int kl_edge_costs(long n_pairs, const float* probs, const int32_t* pair_alt, const double* alt_conf, double lm_weight,
                  double* cost, void* stream);
size_t kl_edge_decode_out_bytes(int n_edges, int beam_width, long n_tracks, long n_pairs);
int kl_edge_decode(const kl_handle* h, int n_edges, const int32_t* desc, const double* cum_in, const int32_t* alt_len,
                   const int32_t* alt_class, const int32_t* step_off, const int32_t* final_slot,
                   const double* pre_cost, const int32_t* pre_class, const int32_t* pre_slot, const double* cost,
                   const float* pool, int depth_k, double dist, int batch_size, int beam_width, int cap_tracks, long n_tracks,
                   long n_pairs, void* out, size_t out_bytes, void* stream);

/* Squared L2 distances between state vectors of pool slots, for beam history
 * clustering (rating.py:887-916): out[i] = || pool[a[i]][k] - pool[b[i]][k] ||^2
 * for state entry k (0 = h1, 1 = c1, ...). */
int kl_state_dist2(const kl_handle* h, int n, const float* pool, const int32_t* a, const int32_t* b, int k,
                   float* out, void* stream);

/* Per-launch timing of the recurrence kernels with HIP events on the caller's
 * stream (used by bench.py for the roofline figure).  While enabled, windows are
 * issued eagerly and the recurrence launches are bracketed by event pairs: each
 * whole-window persistent scan launch, or -- on the launch-per-step path -- runs of
 * 8 consecutive steady-state step launches.  kl_trace_read (after a stream
 * synchronise) returns how many launches were timed, their summed duration and
 * whether they were persistent scans (then also the LSTM contraction FLOPs one such
 * launch carries); kind 0 = forward, 1 = backward recurrence. */
int kl_trace_enable(kl_handle* h, int on);
int kl_trace_read(kl_handle* h, int kind, int* n_launches, float* total_ms, int* persistent,
                  double* flops_per_launch);
/* name of the kernel whose launches kind 0 (forward) / 1 (backward) timed, as rocprofv3 lists it */
const char* kl_trace_kernel_name(kl_handle* h, int kind);

/* Test hooks: the bare contraction kernels on caller buffers. */
int kl_test_gemm_tn(const uint16_t* A, const uint16_t* B, void* C, const float* bias, int M, int N, int K, long lda,
                    long ldb, long ldc, int out_mode, int splits, void* stream);
/* the weight-gradient contraction with a K-major A operand: C[m][n] (or C[n][m] if c_transposed) +=
 * sum_k A_km[k][m] * B[n][k] (b_km: B_km[k][n]); KL_ERR_SHAPE where it does not apply (M % 256, K % 64; K % 32 with
 * b_km and N a multiple of 256, the shapes of the 256 x 256 tile) */
int kl_test_gemm_an(const uint16_t* A_km, const uint16_t* B, float* C, int M, int N, int K, long lda_km, long ldb,
                    long ldc, int c_transposed, int b_km, void* stream);
/* ... and a second product over the same A in the same launch: C2 (+)= A_km^T . B2^T, B2 in the layout b_km names, N a
 * multiple of 128 (B2 null: the single product).  The 256 x 256 tile serves the pair where N and N2 are multiples of 256. */
int kl_test_gemm_an2(const uint16_t* A_km, const uint16_t* B, float* C, int M, int N, int K, long lda_km, long ldb, long ldc,
                     int c_transposed, const uint16_t* B2, float* C2, int N2, long ldb2, long ldc2, int c_transposed2, int b_km,
                     void* stream);
/* Where kl_test_gemm_tn would take a call, decided on the host from the same arguments (c_addr: the address C would have,
 * has_bias: whether a bias is given) and the same KL_GEMM_* switches; nothing is launched and no device is needed.
 * Returns 0 = KL_ERR_SHAPE, 1 = long split-K (256 x 128 ring, K >= 8192, accumulating), 2 = persistent workgroups,
 * 3 = long, one 256 x 128 tile per workgroup, 4 = its 64 x 128 tile, 5 = gemm_tn_kernel with 64-row tiles, 6 = with 128-row
 * tiles, 7 = an empty product (M, N or K <= 0: the call answers 0 and launches nothing); *eff_splits (optional): the K
 * splits the launch would run with. */
int kl_test_gemm_tn_route(int M, int N, int K, long lda, long ldb, long ldc, int out_mode, int splits, size_t c_addr, int has_bias,
                          int* eff_splits);
/* ... and kl_test_gemm_an (N2 = 0) / kl_test_gemm_an2 (N2 > 0): 0 = not applicable (KL_ERR_SHAPE), 1 = the 256 x 128 tile,
 * 2 = the wide form (256 x 256; its ring depth is the LDS grant's answer and not reported), 3 = an empty product;
 * *rows_per_split (optional): the rows of K one split takes. */
int kl_test_gemm_an_route(int M, int N, int N2, int K, long lda_km, long ldb, long ldb2, int b_km, int* rows_per_split);
/* layer 0's table gradients as segment sums over the time-major rows r = t * B + b of dZ [T*B][ld] (bf16; cols a multiple
 * of 8): dEK[v][cols] = sum of the rows with idx[b][t] == v in [0, V), dCtxK[c][cols] = sum of those with
 * ctx[b][t][0] == c in [0, R) (ctx is [B][T][n_ctx]; n_ctx == 0: no context table).  Ids outside their range are dropped,
 * each table on its own.  Both tables are f32, row-major, and zeroed by the call; ws (16-byte aligned,
 * kl_test_segment_sums_ws_bytes) needs no preparation.  kl_test_segment_sums_share: the sorted rows one wave of the gather
 * pass takes.  KL_ERR_SHAPE beyond 65535 (V + 1) * (R + 1) pairs. */
size_t kl_test_segment_sums_ws_bytes(int B, int T, int n_ctx, int V, int R);
int kl_test_segment_sums_share(int B, int T);
int kl_test_segment_sums(const uint16_t* dZ, long ld, int B, int T, int cols, const int32_t* idx, const int32_t* ctx, int n_ctx,
                         int V, int R, float* dEK, float* dCtxK, void* ws, void* stream);
int kl_test_thin_gemm(const float* A, long lda, const uint16_t* WT_hi, const uint16_t* WT_lo, long ldw, int M, int N,
                      int K, float* C, long ldc, int split, void* stream);
/* ... with every form of the operand: A f32 or (a_is_f32 = 0) bf16, an optional gather of A's rows (row_index, int32 on the
 * device: output row r contracts A row row_index[r]) and an optional bias[N], added once */
int kl_test_thin_gemm_ex(const void* A, long lda, int a_is_f32, const int32_t* row_index, const uint16_t* WT_hi, const uint16_t* WT_lo,
                         long ldw, int M, int N, int K, float* C, long ldc, const float* bias, int split, void* stream);
/* The output layer of a training window (logits, softmax, clipped cross-entropy, accuracy, dlogits, dH) on caller buffers:
 * each call is the launcher of one kernel family with its own applicability rule, KL_ERR_SHAPE before anything is launched
 * where it does not apply.  Rows are time-major (r = t * B + b), tgt is [B][T] (-1 = padded position, < -1 = dummy stream),
 * dlogits bf16 [rows][ld_dl] (columns from V on written as zeros), rowstat f32 [rows][2] = (loss, hit) per row, both
 * already scaled by inv_count.
 *   kl_test_softmax_ce      softmax over f32 logits [rows][ld] (strided kernel, or the one-pass kernel for V <= 256 with V,
 *                           ld, ld_dl multiples of 4 and ld_dl <= 256); rowstat is written only with loss_acc != NULL, and
 *                           loss_acc[0], [1] += the sums over the rows (the rowstat reduction)
 *   kl_test_logits_ce_ws    width 512, V = 256: X bf16 [B*T][512], E bf16 [256][512]; B*T >= 8192, a multiple of 32
 *   kl_test_logits_ce_w128  width 128: X bf16 [B*T][128], E bf16 [Vp][128] and ET bf16 [128][Vp] with zeros beyond V,
 *                           V <= Vp <= 256, Vp a multiple of 32; also writes dH f32 [B*T][128] = dlogits . E
 *   kl_test_dh_ws           width 512, Vp = 256: dH bf16 [M][512] = dlogits [M][256] . ET^T, ET bf16 [512][256];
 *                           M >= 4096, a multiple of 32 */
int kl_test_softmax_ce(float* logits, long ld, int rows, int V, const int32_t* tgt, int B, int T, float inv_count, uint16_t* dlogits,
                       long ld_dl, float* rowstat, float* loss_acc, int last_only, void* stream);
int kl_test_logits_ce_ws(const uint16_t* X, const uint16_t* E, const int32_t* tgt, uint16_t* dlogits, float* rowstat, int B, int T,
                         float inv_count, int last_only, void* stream);
int kl_test_logits_ce_w128(const uint16_t* X, const uint16_t* E, const uint16_t* ET, const int32_t* tgt, uint16_t* dlogits, float* dH,
                           float* rowstat, int B, int T, int V, int Vp, float inv_count, int last_only, void* stream);
int kl_test_dh_ws(const uint16_t* dlogits, const uint16_t* ET, uint16_t* dH, long M, void* stream);
/* The embedding regularisers of a training window on caller buffers, one table X f32 [R][D] per call: mode 0 the
 * characters' rule, mode 1 the context tables'.  gX [R][D] += the gradient, loss_acc[2] += the value (loss_acc[0], [1] are
 * not touched); scratch: 3 * D + R + 8 floats.  The window's own launcher with that table alone (a character table without
 * context tables, or a context table without characters); KL_ERR_SHAPE where it refuses the shape. */
int kl_test_regulariser_grads(const float* X, int R, int D, int mode, float* gX, float* loss_acc, float* scratch, void* stream);
/* the selection kernel of kl_rate_window_alts alone: f32 logits [rows][ld], time-major (r = t * B + b, rows == B * T,
 * ld >= V), tgt [B][T]; results batch-major as kl_rate_window_alts describes them (tprob and rank may be NULL).  The
 * register form for V <= 256 with V and ld multiples of 4 (logits 16-byte aligned), the strided form for any other V. */
int kl_test_rate_topk(const float* logits, long ld, int rows, int V, const int32_t* tgt, int B, int T, int K,
                      float* tprob, int32_t* alt_id, float* alt_p, int32_t* rank, void* stream);

/* Test hook: where the handle's most recent kl_train_window of B streams x T steps on workspace ws left what its recurrence
 * scans wrote, and how to read it.  All arrays are time-major with the padded width W = `width`: row r = block * B + b.
 *   off_H   bf16 [(T+1)B][W]   outputs, block 0 = the carried-in h, block t + 1 = step t
 *   off_C   f32  [(T+1)B][W]   cell states, block 0 = the carried-in c; with c_in_cb only blocks 0 and T are written
 *   off_Cb  bf16 [(T+1)B][W]   cell states as the backward scan read them (c_in_cb only)
 *   off_G   bf16 [TB][4W]      gate activations i, f, c, o: [4][W] per row, or [W][4] with g_interleaved
 *   off_dZ  bf16 [TB][4W]      gradients of the gate pre-activations, always [4][W] per row
 *   off_Hd  bf16 [TB][W]       layer l's outputs times its dropout mask, row t * B + b = step t, as the layer above, the output
 *                              layer and the dK product of the layer above read them; 0 where the layer has none (layer 0, or
 *                              a window without masks).  Always the row-major array: where the window's weight gradients
 *                              contract over the transposed copies the wide forward scans write (KL_WG_SCAN_T), the dK
 *                              product reads that copy of the same numbers, which the view does not report.
 * Byte offsets into ws, per layer.  The rounding points the window's plan chose: p_bf16_mask bit l -- layer l's gate inputs
 * from the input side (x . K + b) passed through bf16 rows; dh_bf16 -- the gradient from above (output layer and the layer
 * above) passed through bf16 rows; c_in_cb -- the backward scan read bf16 cell states.  scan2_rows: rows per forward phase of
 * the second-generation wide scans (0: another family).  Nothing is launched or allocated: the answer was noted when the
 * window's launch sequence was built, so it also holds for a window that was a replayed graph.  KL_ERR_STATE if no
 * training window of that shape has run on ws.
 * The weight-gradient stage behind the scans: wg_route = KL_WG_* bits, exactly one of the first three; wg_pair_mask bit l --
 * layer l's dU and dK came from one paired launch; wg_db_scan_mask bit l -- layer l's bias gradient was summed by its backward
 * scan from the f32 values (else by a column sum over the stored bf16 dZ).
 * The output layer in front of them: off_dlogits -- bf16 [TB][ld_dlogits], ld_dlogits = the vocabulary padded to the table
 * rows Vp, row t * B + b = step t: the gradient of the logits as the output-layer kernels stored it and as dH and dE read it
 * (columns from V on are zeros); a region of its own in the workspace, intact when kl_train_window returns.  out_route =
 * KL_OUT_* bits: which of the output-layer kernel families ran, and which form of dlogits the dE product contracted over. */
#define KL_WG_KMAJOR 1     /* products read dZ and the activations as the scans wrote them (K-major plan) */
#define KL_WG_SCAN_T 2     /* ... contract over the transposed outputs the wide forward scans wrote */
#define KL_WG_TRANSPOSE 4  /* ... over explicit transposes into buffers padded to a multiple of 8 rows */
#define KL_WG_SEGSUM 8     /* layer 0: sorted segment sums for the characters and the first context variable (else one-hot products) */
#define KL_WG_PAIR_CTX 16  /* layer 0: the first context variable's one-hot product shared a launch with the characters' */
#define KL_OUT_LOGITS_WS 1    /* logits, softmax, CE and dlogits in one kernel (width 512, V = 256; else GEMM + softmax, or the next) */
#define KL_OUT_LOGITS_W128 2  /* ... the width-128 kernel, and dH came with it */
#define KL_OUT_DH_WS 4        /* dH by the width-512 kernel (else with the logits, or a GEMM) */
#define KL_OUT_DE_KMAJOR 8    /* dE contracted over dlogits as stored (else over its explicit transpose) */
typedef struct kl_window_view {
  int32_t depth, width, B, T;
  int32_t g_interleaved, c_in_cb, dh_bf16, p_bf16_mask, scan2_rows, wg_route, wg_pair_mask, wg_db_scan_mask, out_route, reserved[3];
  uint64_t off_H[16], off_C[16], off_Cb[16], off_G[16], off_dZ[16], off_Hd[16];
  uint64_t off_dlogits, ld_dlogits;
} kl_window_view;
int kl_test_window_view(const kl_handle* h, int B, int T, const void* ws, kl_window_view* out);

/* Test hook: which scan family ran the handle's most recent INFERENCE-layout window of B streams x T steps on workspace ws
 * in the handle's current precision -- kl_forward_window on a workspace of kl_window_workspace_bytes(h, B, T, 0), or
 * kl_rate_window / kl_rate_window_alts, which carve the same window at the start of theirs --, and where it left what it wrote.
 * All arrays are time-major with the padded width W = `width`: row r = block * B + b.
 *   off_H    f32  [(T+1)B][W]   outputs, block 0 = the carried-in h, block t + 1 = step t
 *   off_C    f32  [(T+1)B][W]   cell states, block 0 = the carried-in c; block T = the carried-out c; the blocks between are
 *                               written only with c_every_step (the persistent scans keep c in registers)
 *   off_Xhi, off_Xlo  bf16 [(T+1)B][W]   the (hi, lo) planes the split-precision scans exchange: hi = RNE bf16 of h, lo = RNE
 *                               bf16 of h - hi, every block 0 .. T.  0 where the finishing family leaves no planes (the launch
 *                               per step wavefront reads the f32 rows; bf16 precision has none)
 *   off_P1   f32  [TB][4W]      gate inputs x . K_l + b_l of layer p1_layer for all steps, gates i, f, c, o [4][W] per row: the
 *                               one buffer every layer's input side passes through, so it holds the LAST layer that used it
 *                               (0: the rows gathered from the look-up tables; the top layer where the layers run one after the
 *                               other)
 * Byte offsets into ws, per layer.  family = the KL_FWD_* family that finished the window; passed_mask = the families that issued
 * launches for it and then handed it on (their arrays are overwritten by the finishing family).  ring_mask / thin_mask bit l:
 * layer l's gate inputs came from the three products of the split (hi.hi + b, lo.hi, hi.lo) on the ring GEMM over the planes
 * of the layer below / from the thin split-precision GEMM over its f32 rows (KL_FWD_SPLIT_LAYERS only; in every other family
 * the scan contracts the inputs itself).  handoff = how the scan's workgroups hand rows over.  precision = KL_PREC_*.
 * Each value is noted by the family itself while the window's launch sequence is built, so it also holds for a window that was
 * a replayed graph; nothing is launched or allocated.  KL_ERR_STATE if no such window has run on ws. */
#define KL_FWD_SPLIT_PAIRS 1     /* width 1024, up to 32 streams: two layers per launch, eight units per workgroup */
#define KL_FWD_SPLIT_LAYERS 2    /* width 1024, up to 256 streams: one layer per launch, its input side from one product over all steps */
#define KL_FWD_SPLIT_FUSED 4     /* all layers and steps in one persistent launch */
#define KL_FWD_WAVEFRONT 8       /* a launch per step, layers as a wavefront */
#define KL_FWD_HANDOFF_NONE 0
#define KL_FWD_HANDOFF_SENTINELS 1   /* the published rows themselves, armed with a pattern no value takes */
#define KL_FWD_HANDOFF_COUNTERS 2
typedef struct kl_forward_view {
  int32_t depth, width, B, T;
  int32_t family, passed_mask, ring_mask, thin_mask, handoff, c_every_step, precision, p1_layer, reserved[4];
  uint64_t off_H[16], off_C[16], off_Xhi[16], off_Xlo[16];
  uint64_t off_P1;
} kl_forward_view;
int kl_test_forward_view(const kl_handle* h, int B, int T, const void* ws, kl_forward_view* out);

/* Test hook: where kl_bind carved every operand array the kernels read instead of the parameter vector, and which of them
 * match the bound parameters now.  Byte offsets into the bound derived buffer; per-layer arrays have 16 entries, per-context
 * arrays 8.  W = width, V = voc_size, Vp = V padded to the table rows; bf16 unless stated; gate column order i, f, c, o.
 *   UT_hi/lo, KT_hi/lo [4W][W]  U_l^T, K_l^T (layer 0: rows [0, W) of K0), hi = RNE bf16, lo = RNE bf16 of the remainder
 *   Un, Kn [W][4W]              the same weights untransposed (hi)
 *   E_hi/lo [Vp][W], ET [W][Vp] the embedding, zeros beyond V
 *   EK f32 [V][4W]              E . K0[:W];   CtxK[n] f32 [ctx_vocab][4W] = Ctx_n . K0[W + n ctx_dim ..]
 *   KTp[l] [4W][W], bp[l] f32 [4W]   row u*4+g <- g*W+u of KT_hi[l] / b_l, layers from 1 on (mask_il bit l)
 *   EKp f32 [V][W][4] = EK + b_0, CtxKp[n] f32 [ctx_vocab][W][4]   the same interleave of the tables
 *   comb [V ctx_vocab][W][4]    bf16(EKp[v] + CtxKp[0][c]); carved only where has_comb
 *   UF[l], KF[l] (mask_KF bit l: layers from 1 on), EF   fragment-major [rows/16][W/32][planes][64][8] of UT, KT, E: one plane
 *                               (hi) in bf16 precision, two (hi, lo) in split precision
 *   WTcat[l] [4W][3 K_l]        blocks [hi | hi | lo], K_0 = W (U^T), K_l = 2W (K^T then U^T); bf16 precision writes block 0 only
 *   WTperm[l]                   WTcat[l] with row g*W+u at (u/32)*128 + g*32 + u%32
 *   Ecat [Vp][3W]               [hi | hi | lo] of E, zeros beyond V; bf16 precision writes block 0 only
 * An offset is meaningful only where its mask says the array is carved (has_comb, mask_il, mask_KF; everything else always is).
 * current = KL_DV_* bits: the groups written from the bound parameters by the last kl_prepare / kl_adam_step or built
 * since.  The library cannot see a caller's own writes to the parameter vector: after those, kl_prepare is due as ever.
 * Nothing is launched or allocated.  KL_ERR_STATE before kl_bind. */
#define KL_DV_EAGER 1        /* UT_hi, KT_hi, Un, Kn, E_hi, ET, EK, CtxK */
#define KL_DV_LO 2           /* UT_lo, KT_lo, E_lo: written in split precision only */
#define KL_DV_INTERLEAVED 4  /* KTp, bp, EKp, CtxKp: written in bf16 precision at width 512 with the second-generation scans on */
#define KL_DV_INC 8          /* UF, KF, EF: built on the first incremental step after a change of the operands */
#define KL_DV_BIG 16         /* WTcat, WTperm, Ecat: built on the first step that takes the gather + GEMM path */
#define KL_DV_COMB 32        /* comb: built by every window that gathers from it */
typedef struct kl_derived_view {
  int32_t depth, width, voc_size, Vp, n_ctx, ctx_vocab, ctx_dim, precision;
  int32_t current, has_comb, mask_il, mask_KF, reserved[4];
  uint64_t off_UT_hi[16], off_UT_lo[16], off_KT_hi[16], off_KT_lo[16], off_Un[16], off_Kn[16];
  uint64_t off_KTp[16], off_bp[16], off_UF[16], off_KF[16], off_WTcat[16], off_WTperm[16];
  uint64_t off_CtxK[8], off_CtxKp[8];
  uint64_t off_E_hi, off_E_lo, off_ET, off_EK, off_EKp, off_comb, off_EF, off_Ecat;
  uint64_t bytes;      /* kl_derived_bytes */
} kl_derived_view;
int kl_test_derived_view(const kl_handle* h, kl_derived_view* out);
/* Test hook: build the lazily built operand groups now, each by the launches its first user issues -- mask bit 0 the
 * incremental step's (KL_DV_INC), bit 1 the gather + GEMM path's (KL_DV_BIG), bit 2 the table of all sums (KL_DV_COMB).
 * KL_ERR_STATE before kl_prepare, KL_ERR_ARG for an empty mask or other bits, KL_ERR_SHAPE for bit 2 where comb is not
 * carved or the interleaved tables it sums are not current; all before anything is launched. */
int kl_test_prepare_lazy(kl_handle* h, int mask, void* stream);
/* Test hook, host only: the route a step of n hypotheses takes on this handle -- the plan kl_step_batch (host = 0; has_ws:
 * a workspace of at least kl_step_workspace_bytes(h, n) is passed) or kl_step_batch_host (host = 1; has_ws is ignored, its
 * workspace always holds the step's) itself asks before it launches, not a copy of its rules.
 *   layers     KL_STEP_TILES: a launch per layer on tile_rows x 128 tiles, XCD partition px x py (0, 0: none);
 *              KL_STEP_CELLS: a launch per layer of the 16-unit cell kernel with nmt[l] row tiles per workgroup, gen[l] = the
 *              instantiation for widths 64 and 128; KL_STEP_GEMM_FUSED / KL_STEP_GEMM_PLAIN: gather + GEMM with the cell
 *              in its epilogue / + a gates kernel; KL_STEP_THIN: a launch per layer of the thin forward-step kernel
 *   out        KL_STEP_OUT_FUSED: logits + softmax in one launch; KL_STEP_OUT_THIN: thin GEMM + softmax (host = 1 with the
 *              indices in the kernel arguments: the softmax is the delivering launch's); KL_STEP_OUT_BIG: gather + GEMM + softmax
 *   idx        KL_STEP_IDX_DEVICE: the caller's device arrays; KL_STEP_IDX_KERNARG: in the kernel arguments, provided every
 *              index value of the call is in range (else the packed copy); KL_STEP_IDX_PACKED: one copy of the packed
 *              indices, then the device-pointer step
 *   gathered   layer 0's gate inputs are gathered into the workspace first (n_ctx != 1)
 *   lo         the lo planes of states and weights are used (split precision; 0 before kl_prepare)
 * Fields of other routes are 0.  Nothing is launched or allocated.  KL_ERR_STATE before kl_bind, KL_ERR_ARG for n < 1,
 * KL_ERR_WORKSPACE where the step would return it (n_ctx != 1 without a workspace). */
#define KL_STEP_TILES 1
#define KL_STEP_CELLS 2
#define KL_STEP_GEMM_FUSED 3
#define KL_STEP_GEMM_PLAIN 4
#define KL_STEP_THIN 5
#define KL_STEP_OUT_FUSED 1
#define KL_STEP_OUT_THIN 2
#define KL_STEP_OUT_BIG 3
#define KL_STEP_IDX_DEVICE 1
#define KL_STEP_IDX_KERNARG 2
#define KL_STEP_IDX_PACKED 3
typedef struct kl_step_route {
  int32_t layers, out, idx, lo, gathered, depth;
  int32_t tile_rows, px, py;
  int32_t nmt[16], gen[16];
  int32_t reserved[7];
} kl_step_route;
int kl_test_step_route(const kl_handle* h, int n, int has_ws, int host, kl_step_route* out);

#ifdef __cplusplus
}
#endif
#endif /* KERASLM_HIP_H */
