/* mst_amd.h — C ABI of libmst_amd.so, the MI355X (gfx950) hot path of music-style-transfer.
 *
 * The reference (marcinp7/music-style-transfer) is pure Python and has no FFI; the boundary
 * this library sits behind is the Python surface of style/model.py.  Each entry point names
 * the reference interface it replaces (paths relative to the reference root).  A maintainer
 * binds these with ctypes; no torch types cross the boundary — only raw
 * device pointers, sizes and a hipStream_t.
 *
 * Conventions: every function returns 0 on success and a negative mst_status otherwise and
 * never throws; all work is enqueued on `stream` (no host synchronisation, no allocation in
 * the launch path — graph-capturable); all tensors are fp32, contiguous, device-resident.
 */
#ifndef MST_AMD_H
#define MST_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MST_OK = 0,
    MST_ERR_ARG = -1,          /* null pointer / bad size */
    MST_ERR_UNSUPPORTED = -2,  /* layer width outside the instantiated kernels */
    MST_ERR_LAUNCH = -3,       /* hipGetLastError() after a launch */
    MST_ERR_ALLOC = -4,
} mst_status;

/* Layer widths = the constructor arguments at train-model.py:54-60 + style/data.py:19-31,
 * clip shape = (channel, bar, beat) of prepare_input's tensors (style/data.py:130-156). */
typedef struct {
    int32_t C, R, T;            /* pitched channels, bars, beats per bar (batch is always 1) */
    int32_t beat, bar, nrf;     /* beat_size, bar_size, n_rhythm_features */
    int32_t style, melody, rhythm;
    int32_t instr;              /* instrument_size (51) */
    int32_t n_instruments;      /* 41 */
    int32_t has_unpitched;      /* unpitched_channels is not None */
    int32_t clips;              /* independent clips of this shape carried by every launch (0 or 1 = one clip).
                                 * The reference is strictly batch 1 and sums gradients over iter_size songs
                                 * (train-model.py:95,126,151-153); K clips here = K such iterations at the same
                                 * parameters: per-clip combine / LSTM chains / loss tree, parameter gradients summed. */
} mst_dims;

enum { MST_STAGE_EXTRACT = 1, MST_STAGE_INFO = 2, MST_STAGE_APPLY = 4, MST_STAGE_ALL = 7 };

/* Loss leaves, in the key order of get_total_loss's nested dict flattened with '_'
 * (style/model.py:944-996, train-model.py:148). Unpitched leaves are NaN when absent. */
enum {
    MST_L_TOTAL = 0,
    MST_L_CH_TOTAL, MST_L_P_TOTAL, MST_L_P_NOTES, MST_L_P_VELOCITY, MST_L_P_DURATION, MST_L_P_ACCIDENTALS,
    MST_L_U_TOTAL, MST_L_U_NOTES, MST_L_U_VELOCITY, MST_L_U_DURATION,
    MST_L_SI_TOTAL, MST_L_SI_INSTRUMENTS, MST_L_SI_MODE, MST_L_SI_BPM,
    MST_N_LOSSES
};

typedef struct mst_plan mst_plan;
typedef void* mst_stream;       /* hipStream_t */

/* ---- parameter layout: replaces model.parameters()/state_dict() ordering
 * (style/model.py:36-75,102-126,144-177,203-250,301-344,384-416,446-511,582-622,678-701,727-749).
 * All parameters live in ONE flat fp32 buffer in model.parameters() order. */
int32_t mst_param_count(const mst_dims* d);
int64_t mst_param_floats(const mst_dims* d);
/* i-th tensor: state_dict name, flat offset, shape (up to 3 dims). */
int32_t mst_param_info(const mst_dims* d, int32_t i, char* name, int32_t name_cap,
                       int64_t* offset, int32_t* ndim, int32_t shape[3]);

/* MST_OK when the HIP kernels are instantiated for the layer widths in `d` (the note-level kernels exist for
 * melody_size 4, 8, 12 and 16 — a multiple of 4 from 4 to 16 — with the reference's derived widths; the hidden size of each of the seven LSTMs is at most 1024),
 * MST_ERR_UNSUPPORTED otherwise.  mst_plan_create applies the same rule, so the Python constructors fail early
 * instead of at the first forward. */
int32_t mst_widths_supported(const mst_dims* d);

/* ---- plan: static launch schedule + device-side descriptors for one mst_dims. */
typedef struct {
    int32_t gemm_tile;          /* 0 = choose from the clip count (64x64 tiles from 6 clips per launch on, else 32x32
                                 * split-K tiles); 32 / 64 = force that tiling (experiments, parity tests) */
    int32_t no_merge;           /* 1 = one launch per scheduled member (profiling aid); 0 = merge a dependency level's
                                 * launches of one kernel */
    int32_t gemm_run;           /* 64x64 tiling: output tiles one workgroup walks back to back; 0 = choose (1..8, keeping >= ~4096
                                 * workgroups per launch) */
    int32_t tile_r0, tile_rows; /* bar tiling of ONE clip over several ranks (BASELINE.json configs[4]): this plan computes
                                 * the per-position work of bars [tile_r0, tile_r0 + tile_rows) of the mst_dims.R bars; the bar-level
                                 * chains run replicated.  tile_rows = 0: not tiled.  Run with mst_tiled_phase (clips must be 1);
                                 * `pitched` / `unpitched` are then the tile's bars only: (1,C,tile_rows,T,10,56,5), (1,1,tile_rows,T,10,47,2) */
    int32_t lstm_flavour;       /* StyleEncoder.bars_lstm (H = 192, style/model.py:152,179-181): 0 = choose (the 12-workgroup-per-clip
                                 * kernels when all of a launch's workgroups fit the device at once with one workgroup slot per CU to spare,
                                 * else one workgroup per sequence); 1 = always one workgroup per sequence (use it when other kernels are
                                 * meant to run beside a batched plan); 2 = the 12-workgroup kernels with an injected exchange fault
                                 * (tests of the mst_plan_status path only) */
    int32_t dense_flavour;      /* large dense nn.Linear layers of plans on the 64x64 tiling (lin.hip: all clips as rows of one launch, 2 x 2-blocked
                                 * MFMA tiles): 0 = choose (layers of >= 512 rows and >= 4 MFLOP per clip with more than 32 outputs), 1 = never, 2 = every eligible layer (parity tests
                                 * at small sizes) */
    int32_t branches;           /* 1 = spread the launches of the whole-model passes over the caller's stream + 3 side streams along the dependency
                                 * DAG (event waits where a dependency crosses streams); 0 = one stream (default).  An experiment that LOST on
                                 * MI355X (ROCm 7.2), kept for the record and for its parity test: one bench clip, eager launches 0.85 ms per
                                 * step against 0.49; a replayed hipGraph 875 us per iteration against 812 (a graph with parallel branches pays
                                 * ~5 us per node boundary and per cross edge, a single chain ~2 us per boundary: tools/probe/capture_probe.cpp);
                                 * torch.cuda.graph's capture_end crashes on such captures, so the Python binding refuses them. */
} mst_plan_options;
mst_plan* mst_plan_create(const mst_dims* d, int32_t* status);                       /* default options */
mst_plan* mst_plan_create_ex(const mst_dims* d, const mst_plan_options* opt, int32_t* status);
int32_t mst_plan_gemm_tile(const mst_plan* p);                                       /* 32 or 64 */
void mst_plan_destroy(mst_plan* p);
int64_t mst_plan_workspace_floats(const mst_plan* p);
/* Named tensor inside the workspace: activation offset, gradient offset, element count.
 * Names: "instr","mode","bpm","style","melody","rhythm","instruments_pred","mode_pred",
 * "bpm_pred","pitched_pred","unpitched_pred","pitched_beats","pitched_bars",... */
int32_t mst_plan_tensor(const mst_plan* p, const char* name, int64_t* off, int64_t* goff, int64_t* numel);
int32_t mst_plan_launch_count(const mst_plan* p, int32_t stage_mask, int32_t backward);
/* out = {clips, activation floats per clip, scratch floats per clip, offset of the gradient arena}.
 * Clip k's copy of a named tensor sits k * out[1] floats after clip 0's (mst_plan_tensor offsets). */
int32_t mst_plan_layout(const mst_plan* p, int64_t out[4]);

/* ---- device health.  Kernels whose workgroups wait for each other (the 12-workgroup StyleEncoder LSTM) cannot report a
 * failure through a return code: the launch has long returned.  They OR a bit into a status word inside the workspace
 * (named tensor "device_status", first element, int32) and produce NaNs from then on; the word is sticky.  mst_plan_status
 * synchronises `stream`, copies the word to *status and, with clear != 0, resets it.  A training loop that reads its losses back
 * every N iterations checks it at the same moment (style/train.py LossLog.flush).  No reference counterpart: the reference has
 * no device-side synchronisation of its own. */
enum { MST_DEV_OK = 0, MST_DEV_LSTM_TIMEOUT = 1 /* a granule of the LSTM exchange did not arrive within 0.2 s */ };
int32_t mst_plan_status(const mst_plan* p, float* ws, int32_t clear, int32_t* status, mst_stream stream);

/* ---- forward: StyleTransferModel.extract_style / predict_song_info / apply_style / forward
 * (style/model.py:751-793), selected by stage_mask. `pitched` (1,C,R,T,10,56,5) and
 * `unpitched` (1,1,R,T,10,47,2) are borrowed for the call; small inputs and stage-boundary
 * tensors are read from / written to their workspace slots (mst_plan_tensor). */
int32_t mst_forward(const mst_plan* p, int32_t stage_mask, const float* params, float* ws,
                    const float* pitched, const float* unpitched, mst_stream stream);

/* ---- backward of the same stages (what loss.backward() does, train-model.py:126).
 * Reads output gradients from the workspace gradient slots, accumulates parameter gradients
 * into gparams (+=, sum semantics — train-model.py:126,151-153).  Call mst_zero_grads(stage_mask) before it;
 * when a stage runs on its own the caller also writes (or clears) the gradient slots of that stage's outputs and
 * of the stage-boundary tensors "style", "melody", "rhythm". */
int32_t mst_backward(const mst_plan* p, int32_t stage_mask, const float* params, float* gparams,
                     float* ws, const float* pitched, const float* unpitched, mst_stream stream);
int32_t mst_zero_grads(const mst_plan* p, int32_t stage_mask, float* ws, mst_stream stream);
/* Gradient floats per clip that mst_zero_grads(stage_mask) clears: only ranges the plan's first-writer analysis could not
 * prove written before they are read or accumulated into (every other gradient slot's first writer stores). */
int64_t mst_plan_zero_floats(const mst_plan* p, int32_t stage_mask);

/* ---- get_total_loss (style/model.py:935-997) with normalize flag; pointer based so that it
 * also serves the stand-alone Python get_total_loss. n_*_pos = number of note positions
 * (product of all dims but the last). losses: MST_N_LOSSES floats. saved: MST_LOSS_SAVED floats
 * carried to the backward call. partials: scratch of mst_loss_scratch_floats(). */
#define MST_LOSS_SAVED 512
int64_t mst_loss_scratch_floats(void);
int32_t mst_total_loss_fwd(const float* pitched_pred, const float* pitched_target, int64_t n_pitched_pos,
                           const float* unpitched_pred, const float* unpitched_target, int64_t n_unpitched_pos,
                           const float* instr_logits, const float* instr_target, int32_t n_instr,
                           const float* mode_logits, const float* mode_target,
                           const float* bpm_pred, const float* bpm_target,
                           int32_t normalize, float* losses, float* saved, float* scratch, mst_stream stream);
/* grad_losses: MST_N_LOSSES upstream gradients (one-hot on MST_L_TOTAL for loss.backward()).
 * Writes (=) the gradients of every prediction. */
int32_t mst_total_loss_bwd(const float* pitched_pred, const float* pitched_target, int64_t n_pitched_pos,
                           const float* unpitched_pred, const float* unpitched_target, int64_t n_unpitched_pos,
                           const float* instr_logits, const float* instr_target, int32_t n_instr,
                           const float* mode_logits, const float* mode_target,
                           const float* bpm_pred, const float* bpm_target,
                           const float* saved, const float* grad_losses,
                           float* g_pitched, float* g_unpitched, float* g_instr, float* g_mode, float* g_bpm,
                           mst_stream stream);

/* ---- one train-model.py loop body (train-model.py:113-126): forward, total loss,
 * backward; gradients accumulate in gparams. Targets are the inputs (auto-encoder), the
 * instrument target is `used` (n_instruments), bpm target a device float. losses may be null.
 * With mst_dims.clips = K: `pitched` is (K,C,R,T,10,56,5), `unpitched` (K,1,R,T,10,47,2), `losses`
 * K x MST_N_LOSSES, the per-clip small inputs sit in each clip's workspace slice, and gparams
 * receives the SUM over the K clips (= K loop bodies at the same parameters). */
int32_t mst_train_iteration(const mst_plan* p, const float* params, float* gparams, float* ws,
                            const float* pitched, const float* unpitched, float* losses, mst_stream stream);

/* ---- one loop body (train-model.py:113-126) of a clip whose bars are tiled over ranks.  Every rank calls phase 0, 1, ...
 * mst_tiled_phase_count() - 1 on its own plan / workspace / gparams; a phase returns *nx <= MST_MAX_XCHG workspace ranges
 * ws[xoff[q], xoff[q] + xlen[q]) that the host all-reduces (SUM) over the ranks before the next phase — as ONE collective (pack the
 * ranges, reduce, unpack: Plan.tiled_train_iteration); exchanges of one dependency level end the same phase.  Afterwards gparams
 * holds this rank's share of the clip's gradient: all-reduce (SUM) it like in data parallelism (train-model.py:126,151-153), then
 * mst_adam_step.  is_root: exactly one rank passes 1 (it contributes the replicated song-info loss gradients).  losses:
 * MST_N_LOSSES floats, identical on every rank. */
#define MST_MAX_XCHG 8
int32_t mst_tiled_phase_count(const mst_plan* p);
int32_t mst_tiled_phase(const mst_plan* p, int32_t phase, const float* params, float* gparams, float* ws,
                        const float* pitched, const float* unpitched, float* losses, int32_t is_root,
                        mst_stream stream, int64_t xoff[MST_MAX_XCHG], int64_t xlen[MST_MAX_XCHG], int32_t* nx);

/* ---- torch.optim.Adam(lr=.01) + StepLR(200,.9) + zero_grad (train-model.py:89-90,151-154)
 * over the flat buffers. state: 4 floats {step count t, lr_t/(1-b1^t), sqrt(1-b2^t), reserved} kept on the device so that
 * the launch is graph-replayable; lr = lr0 * gamma^(t / step_size). */
int32_t mst_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                      float* state, double lr0, double beta1, double beta2, double eps,
                      int32_t step_size, double gamma, int32_t zero_grad, mst_stream stream);

/* Same step over the SUM of two gradient buffers: the iter_size = 2 accumulation iterations of
 * train-model.py:126,151-153 are independent, so they may run concurrently (two streams, two workspaces,
 * two gradient buffers) and meet here; grads + grads2 equals accumulating in place, bit for bit. */
int32_t mst_adam_step2(float* params, float* grads, float* grads2, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float* state, double lr0, double beta1, double beta2, double eps,
                       int32_t step_size, double gamma, int32_t zero_grad, mst_stream stream);

/* ---- guarded optimizer step: global gradient-norm clipping and the skip of a non-finite step, decided on the device.
 * No reference counterpart: the reference only asserts on a NaN loss (train-model.py:121), and sums its gradients over
 * iter_size songs (train-model.py:126,151-153), so their scale grows with every accumulated clip.
 * The effective gradient is grads, or grads + grads2 formed in fp32 exactly as the step forms it.  Its squares are summed in
 * double: the flat buffer is cut into slices of a fixed element count, one partial per slice in `scratch`
 * (mst_grad_guard_scratch_bytes, 8-byte aligned), and one workgroup adds the partials in a fixed order.  The number of
 * partials depends on n alone; there are no atomics and no workgroup waits for another: the same bits on every run.
 * The gradient buffers need float alignment only.
 *
 * The guarded step, three launches (one more than the plain step), enqueue-only on `stream` (no allocation, no host
 * synchronisation, capturable as a single chain):
 *   norm      = (float)sqrt(sum of squares)
 *   nonfinite = norm is inf or NaN — the test is applied to the fp32 norm, so finite gradients whose norm overflows fp32 count
 *   coef      = min(1, (float)max_norm * (1 / (norm + 1e-6f))) in fp32: max_norm / (total_norm + 1e-6) of
 *               torch.nn.utils.clip_grad_norm_ in the order torch evaluates it (a Python float divided by a tensor is the
 *               reciprocal times the float), so the clipped gradient equals torch's bit for bit given the same norm;
 *               1 when max_norm <= 0 or +inf (no clipping) and 1 when nonfinite
 *   skip      = skip_nonfinite && nonfinite
 * then the step of the plain entry points on the gradient (grads [+ grads2]) * coef, the product rounded to fp32 before it
 * enters Adam's arithmetic: exactly "clip, then the plain step".  With coef = 1 it is the plain step, bit for bit.
 * A skip leaves params, exp_avg, exp_avg_sq and state bit-unchanged — the step count and the StepLR schedule do not
 * advance — and still zeroes grads / grads2 when zero_grad is set.
 * With skip_nonfinite = 0 a non-finite norm gives the plain, unguarded step (coef = 1).  This differs from
 * torch.nn.utils.clip_grad_norm_, whose NaN coefficient would turn every gradient into NaN.
 *
 * guard: MST_GUARD_WORDS device floats, zeroed once by the caller, rewritten by every call:
 *   [0] norm of this call (may be inf / NaN)       [3] calls skipped so far
 *   [1] coefficient applied (1 = not clipped,      [4] calls clipped so far (coef < 1)
 *       0 when skipped)                            [5] largest finite norm so far
 *   [2] 1 if this call was skipped, else 0         [6..7] 0
 * Counts are floats, exact to 2^24, like state[0].
 * MST_ERR_ARG: null pointer other than grads2, n <= 0, step_size <= 0, NaN max_norm, scratch not 8-byte aligned. */
#define MST_GUARD_WORDS 8
int64_t mst_grad_guard_scratch_bytes(int64_t n);   /* bytes of partials for n elements; <= 0 on a bad n */
/* *norm (one device float) = L2 norm of the effective gradient; two launches */
int32_t mst_grad_norm(const float* grads, const float* grads2 /* NULL ok */, int64_t n, void* scratch, float* norm,
                      mst_stream stream);
/* diagnostic, one launch: norms[k] = L2 norm of the effective gradient over [offsets[k], offsets[k] + lengths[k]), for
 * k < count; offsets / lengths are DEVICE arrays; same double accumulation in a fixed order, one workgroup per range */
int32_t mst_grad_norms(const float* grads, const float* grads2 /* NULL ok */, const int64_t* offsets, const int64_t* lengths,
                       int32_t count, float* norms, mst_stream stream);
int32_t mst_adam_step_guarded(float* params, float* grads, float* grads2 /* NULL ok */, float* exp_avg, float* exp_avg_sq,
                              int64_t n, float* state, float* guard, void* scratch, double lr0, double beta1, double beta2,
                              double eps, int32_t step_size, double gamma, double max_norm /* <= 0 or +inf: no clipping */,
                              int32_t skip_nonfinite, int32_t zero_grad, mst_stream stream);

/* ---- hard_output (style/model.py:818-832): n_pos positions x nfeat (5 or 2) features.
 * Like the reference it also zeroes sub-threshold velocities of `x` in place. */
int32_t mst_hard_output(float* x, float* out, int64_t n_pos, int32_t nfeat, mst_stream stream);

/* ---- sparse clip input: build dense note tensors from sorted note records on the device.
 * A piano roll is > 98 % zeros, so a clip travels as records and is expanded here.  For each clip k of n_clips:
 *   cells[k * capacity + i]            flat cell index (C order of the roll without its feature axis), strictly ascending in i
 *   feats[(k * capacity + i) * nfeat]  the cell's nfeat (5 pitched / 2 unpitched) floats
 *   counts[k]                          live records of clip k, read ON THE DEVICE (a captured graph replays with another clip);
 *                                      clamped to [0, capacity]; records beyond it are ignored
 * out: n_clips x n_cells x nfeat floats.  EVERY float is written — the record's value or +0.0 — so the caller never clears the
 * buffer and stale (or NaN) contents of a reused one disappear.  A record whose cell is outside [0, n_cells) is skipped, never
 * stored.  One launch, enqueue-only on `stream` (no allocation, no host synchronisation, capturable), no atomics: bit-reproducible.
 * out needs float alignment only.  MST_ERR_ARG: null pointer, nfeat outside {2, 5}, n_cells < 1 or >= 2^31, n_clips < 1,
 * capacity < 0. */
int32_t mst_clip_scatter(const int32_t* cells, const float* feats, const int32_t* counts, int32_t capacity, int32_t n_clips,
                         int64_t n_cells, int32_t nfeat, float* out, mst_stream stream);

/* ---- windowed clips: K same-shaped clips cut out of differently long songs whose records stay on the device.
 * cells / feats are a POOL holding the records of many songs back to back; win[k] (a DEVICE array, read ON THE DEVICE: a
 * captured graph replays with other songs and other windows) describes clip k:
 *   first, count   the song's records are cells[first, first + count) (and the matching feats rows): the strictly ascending
 *                  flat cell indices of a roll (channels, src_bars, bar_cells); count is clamped at 0, a negative first
 *                  reads as no records
 *   src_bars       bars of that song;  r0  the first bar of the window, may be negative or reach past the end
 * out: n_clips x channels x bars x bar_cells x nfeat floats; out[k, c, r, j, :] is the source cell (c, r0 + r, j) when
 * 0 <= r0 + r < src_bars, else +0.0 — i.e. x[:, r0:r0 + bars] of the dense song, zero-extended.  bar_cells is T*10*56 for a
 * pitched roll and T*10*47 (channels = 1) for an unpitched one.  mst_clip_scatter's promises hold: EVERY float of out is
 * written exactly once (no clearing, stale or NaN contents disappear), nothing outside out is written, out needs float
 * alignment only, no atomics (bit-reproducible), one launch, enqueue-only on `stream`, capturable; a record whose cell lies
 * outside its song's roll is skipped, never stored (a song of 2^31 cells or more reads as silence).  MST_ERR_ARG: null
 * pointer, nfeat outside {2, 5}, n_clips / channels / bars / bar_cells < 1, channels * bars * bar_cells >= 2^31. */
typedef struct { int32_t first, count, src_bars, r0; } mst_window;   /* 16 bytes */
int32_t mst_clip_window(const int32_t* cells, const float* feats, const mst_window* win, int32_t n_clips, int32_t channels,
                        int32_t bars, int64_t bar_cells, int32_t nfeat, float* out, mst_stream stream);

/* ---- rotating song store: one refresh of the pools and tables that mst_clip_window / mst_window_inputs read, as ONE batched,
 * segmented, bit-exact copy.  Everything that varies is read ON THE DEVICE, so the launch arguments are the same for every
 * refresh.  blob (a DEVICE staging buffer of blob_words 32-bit words) holds one refresh:
 *   blob[0]              the segment count n, clamped to [0, max_segments]; blob[1..3] are not read
 *   blob[4 + 4 i ..]     segment i (mst_segment; every field counts 32-bit words)
 *   the payload          behind the header of max_segments segments; src_off counts from the start of the blob
 * Segment i copies `words` words from blob + src_off to (int32_t*)dst[dst] + dst_off, bit for bit (the words travel as integers:
 * NaN payloads and -0.0 survive) — if 0 <= dst < MST_ADMIT_DSTS, dst[dst] != NULL, words >= 0, the source range lies inside
 * [4 + 4 max_segments, blob_words) and the destination range inside [0, dst_words[dst]); otherwise NOTHING of that segment is
 * written.  status[i], for EVERY i < max_segments on EVERY launch: 0 = copied or unused (i >= n), 1 = refused; written with
 * plain stores, never cleared by the caller.  Where source and destination address agree modulo 16 the copy moves 16 bytes at
 * a time between a word-wise head and tail; where they do not it moves words.  Every pointer needs 4-byte alignment only.
 * mst_clip_scatter's promises hold: nothing outside the named destination ranges is written, one launch on a grid sized from
 * the device's compute units, enqueue-only on `stream` (no allocation, no host synchronisation, capturable), no atomics,
 * bit-reproducible.  Destination ranges that overlap within one call are the caller's business.  MST_ERR_ARG, and nothing is
 * launched: a null blob / dst / dst_words / status, max_segments < 1, blob_words < 4 + 4 max_segments, a pointer that is not
 * 4-byte aligned. */
enum { MST_ADMIT_DSTS = 16 };
typedef struct { int32_t dst, dst_off, src_off, words; } mst_segment;   /* 16 bytes, all in 32-bit words */
int32_t mst_store_admit(const int32_t* blob, int64_t blob_words, int32_t max_segments, void* const dst[MST_ADMIT_DSTS],
                        const int64_t dst_words[MST_ADMIT_DSTS], int32_t* status /* max_segments int32 */, mst_stream stream);

/* ---- sparse clip output: the sorted note records of a dense roll, built on the device — the inverse of mst_clip_scatter, so
 * that inference downloads the notes (24 bytes per pitched record) instead of the whole roll.  x: n_cells x nfeat floats.
 *   MST_ROLL_NONZERO  a cell is a record when the float32 BIT PATTERN of any of its features is non-zero (-0.0 and NaN are
 *                     kept); features verbatim.  The inverse of mst_clip_scatter.
 *   MST_ROLL_HARD     hard_output's decisions (style/model.py:818-832), in mst_hard_output's order: feature 0 the duration,
 *                     feature 1 v > .01f ? v : 0, for nfeat == 5 features 2-4 (x[a] == max && x[a] > .1f) ? 1 : 0.  A cell is a
 *                     record when its hard velocity is non-zero (v > .01f; a NaN velocity is dropped); the record carries the
 *                     HARD features.  Unlike mst_hard_output, x is not modified.
 * The roll is cut into mst_roll_slices(n_cells) slices of consecutive cells.  mst_roll_count leaves in ws (mst_roll_slices + 1
 * int32) the number of records in the slices before slice s at ws[s], and the total at ws[slices].  mst_roll_compact, given
 * that ws, writes the record of rank r < capacity to cells[r] (flat cell index, strictly ascending in r) and
 * feats[r * nfeat ...]; records of rank >= capacity are dropped, never stored: nothing outside cells[0, min(total, capacity))
 * and the matching floats is written.  Two launches and one; enqueue-only on `stream` (no allocation, no host synchronisation,
 * capturable); no atomics, no workgroup waits for another: the output is bit-identical run to run.  x needs float alignment
 * only.  MST_ERR_ARG: null pointer, n_cells < 1 or >= 2^31, nfeat outside {2, 5}, mode outside {0, 1}, capacity < 0, x not
 * 4-byte aligned. */
enum { MST_ROLL_NONZERO = 0, MST_ROLL_HARD = 1 };
int64_t mst_roll_slices(int64_t n_cells);      /* slices the kernels cut n_cells into; <= 0 on a bad argument */
int32_t mst_roll_count(const float* x, int64_t n_cells, int32_t nfeat, int32_t mode, int32_t* ws, mst_stream stream);
int32_t mst_roll_compact(const float* x, int64_t n_cells, int32_t nfeat, int32_t mode, const int32_t* ws,
                         int64_t capacity, int32_t* cells, float* feats, mst_stream stream);

/* The batched, strided twins: n_rolls rolls compacted at once, in the record layout mst_clip_scatter consumes.  Roll k is the
 * n_cells x nfeat floats at x + k * roll_stride (the K predictions of a batched plan lie mst_plan_layout's clip stride apart in
 * its workspace); the floats between two rolls are never read.  The 16-byte phase of a roll is its own: roll_stride need not be
 * a multiple of 4.  Modes and record predicates are those above.
 * mst_rolls_count leaves in row k of ws (n_rolls rows of mst_roll_slices(n_cells) + 1 int32) exactly what mst_roll_count leaves
 * for that roll.  mst_rolls_compact, given that ws, writes the record of rank r < capacity of roll k to cells[k * capacity + r]
 * (the cell index within the roll, strictly ascending in r) and feats[(k * capacity + r) * nfeat ...], and the roll's TRUE number
 * of records to counts[k]: the caller sees an overflow, and mst_clip_scatter clamps the count.  Records of rank >= capacity are
 * dropped, never stored: of row k nothing beyond min(counts[k], capacity) records is written, x and ws are read only, and with
 * capacity = 0 only counts is written.  One launch and one scan launch (a workgroup per roll) for the count, one launch for the
 * compaction — the count's first and the compaction's launch once per 65535 rolls, as mst_roll_metrics; enqueue-only on `stream` (no allocation, no host synchronisation,
 * capturable as a single chain); no atomics, no workgroup waits for another: the same bits on every run.  x needs float
 * alignment only.  MST_ERR_ARG, and nothing is launched: null pointer, n_rolls < 1, n_cells < 1 or >= 2^31, n_rolls x slices >=
 * 2^31, nfeat outside {2, 5}, mode outside {0, 1}, capacity < 0, roll_stride < n_cells * nfeat, x not 4-byte aligned. */
int32_t mst_rolls_count(const float* x, int64_t roll_stride, int32_t n_rolls, int64_t n_cells, int32_t nfeat, int32_t mode,
                        int32_t* ws /* n_rolls x (mst_roll_slices(n_cells) + 1) */, mst_stream stream);
int32_t mst_rolls_compact(const float* x, int64_t roll_stride, int32_t n_rolls, int64_t n_cells, int32_t nfeat, int32_t mode,
                          const int32_t* ws, int32_t capacity, int32_t* cells, float* feats, int32_t* counts, mst_stream stream);

/* ---- note metrics: how good are hard_output's decisions?  No reference counterpart: the reference has no validation, and
 * get_total_loss (style/model.py:935-997) reports soft quantities only — its smooth F1 is computed on raw velocities, while the
 * inference driver writes hard_output's decisions (style/model.py:818-832) to MIDI.
 * pred, target: two rolls of n_groups x group_cells cells of nfeat (5 or 2) floats; a group is a run of consecutive cells — for
 * the model's tensors one (clip, channel) of the pitched roll or one clip of the unpitched roll.  out: one record of
 * MST_METRIC_WORDS doubles per group:
 *   [0] cells in the group
 *   [1] n_pred: cells with v_pred > .01f (hard_output's note decision; a NaN velocity is off, as in MST_ROLL_HARD)
 *   [2] n_tgt:  cells with v_tgt > 0.f (the loss's mask)
 *   [3] TP:     both
 *   [4] of the TP cells, those whose three hard accidentals ((x[a] == max && x[a] > .1f) ? 1 : 0, mst_hard_output's operations)
 *       equal the target's three accidentals as floats; 0 for nfeat == 2
 *   [5] sum over the TP cells of fabsf(v_pred - v_tgt)
 *   [6] sum over the TP cells of fabsf(d_pred - fminf(d_tgt, 6.f)) (get_duration_loss's clamp); a NaN duration on a matched
 *       note makes it NaN
 *   [7] 0
 * Counts are exact integers held in doubles; [5] and [6] take the fp32 term, widen it and accumulate in double.
 * The groups are cut into mst_roll_slices(group_cells) slices each; a workgroup owns one slice of one group, streams it from both
 * tensors once and leaves a 32-byte partial in `scratch` (mst_roll_metrics_scratch_bytes, 8-byte aligned); a second launch adds a
 * group's partials in a fixed order.  The number of partials depends on the arguments alone; no atomics, no workgroup waits for
 * another: the same bits on every run.  Two launches per 65535 groups, enqueue-only on `stream` (no allocation, no host
 * synchronisation, capturable as a single chain).  Every word of `out` and nothing beyond it is written; pred and target are
 * read only and need float alignment only, each its own.
 * MST_ERR_ARG: null pointer, nfeat outside {2, 5}, n_groups < 1, group_cells < 1 or >= 2^31, n_groups x slices >= 2^31, pred /
 * target not 4-byte aligned, scratch / out not 8-byte aligned. */
#define MST_METRIC_WORDS 8
int64_t mst_roll_metrics_scratch_bytes(int64_t n_groups, int64_t group_cells);   /* <= 0 on bad arguments */
int32_t mst_roll_metrics(const float* pred, const float* target, int64_t n_groups, int64_t group_cells,
                         int32_t nfeat, void* scratch, double* out, mst_stream stream);

/* ---- one evaluation iteration: mst_train_iteration without its backward half — the whole-model forward, get_total_loss with
 * normalize = 1 against the inputs as targets, and the note metrics of the predictions.  No gradient is formed (there is no
 * gparams argument), `params` is read only.  The small inputs and targets (mode, bpm, instr, used_instruments, bpm_target) sit
 * in the workspace slots mst_train_iteration reads.  With mst_dims.clips = K: losses is K x MST_N_LOSSES (may be null), metrics
 * K x (C + 2) records of MST_METRIC_WORDS doubles per clip: the C pitched channels ("pitched_pred" in the workspace against the
 * borrowed `pitched`), one unpitched record (all zero when the plan has no percussion) and one song-info record:
 *   [0] n_instruments                 [3] instruments with both
 *   [1] instruments with logit > 0    [4] 1 if the first index of the largest mode logit is that of the largest mode target
 *   [2] instruments with target > .5  [5] fabsf(bpm_pred - bpm_target)        [6..7] 0
 * scratch: mst_eval_scratch_bytes(p) bytes of the caller's, 8-byte aligned (the plan's workspace layout is unchanged).  Three
 * launches behind the loss: the two rolls' partials and one finishing launch for every record.  Enqueue-only on `stream`.
 * A tiled plan (tile_rows > 0) gives MST_ERR_UNSUPPORTED. */
int64_t mst_eval_scratch_bytes(const mst_plan* p);
int32_t mst_eval_iteration(const mst_plan* p, const float* params, float* ws, const float* pitched,
                           const float* unpitched, float* losses, double* metrics, void* scratch, mst_stream stream);

/* ---- windowed evaluation: a held-out round over a fixed set of windows of resident songs is N replays of one graph —
 * mst_clip_window x 2, mst_window_inputs, mst_eval_iteration, mst_eval_accumulate — and ONE download of 41 doubles.  No reference
 * counterpart: the reference has no validation.  Both entry points are enqueue-only on `stream` (no allocation, no host
 * synchronisation, capturable as a single chain), one launch each, without atomics and without a workgroup waiting for another:
 * the same bits on every run.
 *
 * mst_window_inputs: rows of a device table into per-clip workspace slots.  `table` is table_rows x row_floats floats (a song's
 * small inputs — mode, bpm, instrument features, used instruments, bpm target — are one row); rows[k] (a DEVICE array of n_clips
 * int32, read ON THE DEVICE as mst_clip_window reads its descriptors: a captured launch serves other songs) names clip k's row;
 * `fields` (HOST memory, read at the call) lists up to MST_ROW_FIELDS pieces of a row and where each goes.  For clip k, field
 * f < fields->n and i < len[f]:
 *     ws[dst[f] + k * clip_stride + i] = table[rows[k] * row_floats + src[f] + i]          copied bit for bit
 * A rows[k] outside [0, table_rows) writes quiet NaNs (0x7fc00000) into that clip's fields instead — the mistake shows in the
 * losses rather than leaving stale inputs — and the table is never read outside its rows.  Every float of the named destinations
 * is written exactly once and nothing else is written; keeping the destinations disjoint is the caller's business (a plan's
 * slots are: mst_plan_tensor, mst_plan_layout).  table and ws need float alignment only.  A field of length 0 names nothing.
 * MST_ERR_ARG, and nothing is launched: null pointer, n_clips / table_rows / row_floats < 1, fields->n outside 1..8, a negative
 * src, len or dst, src + len > row_floats, clip_stride < 0, table / ws not 4-byte aligned. */
#define MST_ROW_FIELDS 8
typedef struct { int32_t n; int32_t src[MST_ROW_FIELDS], len[MST_ROW_FIELDS]; int64_t dst[MST_ROW_FIELDS]; } mst_row_fields;
int32_t mst_window_inputs(const float* table, int32_t table_rows, int32_t row_floats,
                          const int32_t* rows /* DEVICE, n_clips */, int32_t n_clips,
                          const mst_row_fields* fields /* HOST, read at the call */,
                          int64_t clip_stride, float* ws, mst_stream stream);

/* mst_eval_accumulate: acc += the batch that mst_eval_iteration just left in `losses` (n_clips x MST_N_LOSSES) and `metrics`
 * (n_clips x (channels + 2) records of MST_METRIC_WORDS doubles).  Only the first min(max(*live, 0), n_clips) clips count
 * (live: one DEVICE int32, read on the device, so one graph serves full batches and a round's padded last one; NULL = all).
 * The caller zeroes acc once per round.  Words of acc:
 *   [0]        clips counted
 *   [1]        counted clips whose MST_L_U_TOTAL is not NaN (clips with percussion)
 *   [2 + i]    sum of loss leaf i, each float widened to double; the four leaves MST_L_U_TOTAL .. MST_L_U_DURATION are added only
 *              for the clips counted in [1]; any other NaN is a real one and propagates (style.metrics.nanmean_leaves' rule)
 *   [17 .. 25) the pitched record, summed over the counted clips and their `channels` records
 *   [25 .. 33) the unpitched record, summed over the counted clips
 *   [33 .. 41) the song-info record, summed over the counted clips, with 1 added to a record's word 7 before it is added: the
 *              `songs` denominator
 * Every word is a left-to-right float64 sum that starts from the word's value on entry and takes its terms in the order clip
 * 0, 1, ... and, within a clip, channel 0, 1, ...: the bits a host loop of double additions in that order gives.  A word without
 * terms (*live <= 0) keeps its bits.  One workgroup of 64 lanes, lane w < 41 owns word w; nothing outside acc[0, 41) is written.
 * MST_ERR_ARG: a null pointer other than live, n_clips < 1, channels < 1, metrics / acc not 8-byte aligned. */
#define MST_EVAL_ACC_WORDS (2 + MST_N_LOSSES + 3 * MST_METRIC_WORDS)   /* 41 doubles */
int32_t mst_eval_accumulate(const float* losses   /* n_clips x MST_N_LOSSES */,
                            const double* metrics /* n_clips x (channels + 2) x MST_METRIC_WORDS, mst_eval_iteration's */,
                            int32_t n_clips, int32_t channels,
                            const int32_t* live   /* DEVICE, one int32, or NULL = all */,
                            double* acc /* MST_EVAL_ACC_WORDS, 8-byte aligned */, mst_stream stream);

/* ---- batched style transfer: clip k of a batch rendered with the style of clip donors[k] of the same batch, and a score of the
 * swap, without leaving the device.  No reference counterpart: the reference transfers one style onto one song per call
 * (style/style_transfer.py) and has no measure of the result.  Both entry points are one launch, enqueue-only on `stream` (no
 * allocation, no host synchronisation, capturable as a single chain), without atomics and without a workgroup waiting for
 * another: the same bits on every run.
 *
 * mst_clip_gather: rows of `src` (src_rows runs of len floats, src_stride floats apart) into per-clip destinations by a device
 * index.  For clip k < n_clips and i < len:
 *     dst[k * dst_stride + i] = src[idx[k] * src_stride + i]          copied bit for bit
 * idx (a DEVICE array of n_clips int32, read ON THE DEVICE as mst_window_inputs reads its rows: a captured launch serves other
 * donors) may be NULL: idx[k] = k.  An idx[k] outside [0, src_rows) writes quiet NaNs (0x7fc00000) into that clip's len floats
 * instead, and src is not read for it.  Every named float of dst is written exactly once and nothing else is written; src is read
 * only; float alignment only.  src_stride = 0 is allowed (every row is the same run).
 * MST_ERR_ARG, and nothing is launched: a null src or dst; n_clips, src_rows or len < 1; a negative stride; dst_stride < len with
 * n_clips > 1 (the destinations would overlap); the ranges [src, src + (src_rows - 1) * src_stride + len) and [dst, dst +
 * (n_clips - 1) * dst_stride + len) intersecting (a permutation in place is a race: go through a side buffer) or not
 * representable; src / dst not 4-byte aligned; more than 2^31 - 1 chunks of 1024 floats in all. */
int32_t mst_clip_gather(const float* src, int32_t src_rows, int64_t src_stride, float* dst, int64_t dst_stride,
                        const int32_t* idx /* DEVICE int32[n_clips] or NULL = identity */, int32_t n_clips, int64_t len,
                        mst_stream stream);

/* mst_style_sums: the raw material of three cosines per clip.  With x = a + k * a_stride, y = b + idx[k] * b_stride and
 * z = b + k * b_stride (len floats each; idx as above, NULL = identity), the MST_STYLE_SUM_WORDS doubles of out[k] are
 *   [0] sum x.x   [1] sum y.y   [2] sum z.z   [3] sum x.y   [4] sum x.z   [5] sum y.z   [6] len   [7] 0
 * Each sum is a left-to-right float64 sum over i = 0 ... len - 1 that starts from 0; a term is the product of the two floats
 * widened to double, which is exact: the bits a host loop of double additions in that order gives.  One workgroup of 64 lanes
 * per clip, lane w < 6 owns word w.  An idx[k] outside [0, b_rows) makes words 1, 3 and 5 of that clip NaN, a k >= b_rows words
 * 2, 4 and 5; the other words stay right and b is not read outside its rows.  Every word of out[0, n_clips x 8) and nothing
 * beyond it is written; a and b are read only (they may overlap) and need float alignment only.  Quotients and square roots are
 * the host's (style.metrics.style_cosines), so the device result stays bit-checkable.
 * MST_ERR_ARG, and nothing is launched: a null a, b or out; n_clips or b_rows < 1; len < 1 or >= 2^31; a negative stride; a / b
 * not 4-byte aligned; out not 8-byte aligned. */
#define MST_STYLE_SUM_WORDS 8
int32_t mst_style_sums(const float* a, int64_t a_stride, const float* b, int32_t b_rows, int64_t b_stride,
                       const int32_t* idx /* DEVICE int32[n_clips] or NULL = identity */, int32_t n_clips, int64_t len,
                       double* out /* n_clips x MST_STYLE_SUM_WORDS, 8-byte aligned */, mst_stream stream);

/* ---- style bank: a clip rendered with a stored style, a blend of stored styles or the style of a song of another shape, and
 * with the instruments, mode and tempo the model predicts for it, without leaving the device.  The reference's counterpart of
 * mst_info_decide is the host half of apply_style (style/style_transfer.py:101-116); a bank has none.  Each entry point is one
 * launch, enqueue-only on `stream` (no allocation, no host synchronisation, capturable as a single chain), without atomics and
 * without a workgroup waiting for another: the same bits on every run.  Every index array is DEVICE memory, read on the device:
 * a captured launch serves other rows.
 *
 * mst_style_put: per-clip runs of `src` into rows of a bank (bank_rows runs of len floats, bank_stride floats apart).  For clip
 * k < n_clips with 0 <= rows[k] < bank_rows and i < len:
 *     bank[rows[k] * bank_stride + i] = src[k * src_stride + i]          copied bit for bit
 * A rows[k] outside [0, bank_rows) writes nothing for that clip: that is how the repeated windows of a padded batch are dropped.
 * Every named float is written exactly once and nothing else is written — unless two clips name the same row: which of them the
 * row then holds is not defined, and keeping the rows distinct is the caller's business.  src is read only; float alignment only.
 * MST_ERR_ARG, and nothing is launched: a null src, bank or rows; n_clips, bank_rows or len < 1; a negative stride; bank_stride
 * < len with bank_rows > 1 (the rows would overlap); the ranges [src, src + (n_clips - 1) * src_stride + len) and [bank, bank +
 * (bank_rows - 1) * bank_stride + len) intersecting or not representable; a pointer not 4-byte aligned; more than 2^31 - 1
 * chunks of 1024 floats in all. */
int32_t mst_style_put(const float* src, int64_t src_stride, float* bank, int32_t bank_rows, int64_t bank_stride,
                      const int32_t* rows /* DEVICE int32[n_clips] */, int32_t n_clips, int64_t len, mst_stream stream);

/* mst_style_mix: a CSR-weighted sum of bank rows into per-clip destinations.  Clip k owns the entries e = offsets[k] ...
 * offsets[k + 1] - 1 of idx and w (n_entries each; offsets holds n_clips + 1 int32); with x[e] = bank + idx[e] * bank_stride,
 *     dst[k * dst_stride + i] = (((w[e0] * x[e0][i]) + w[e0 + 1] * x[e0 + 1][i]) + ...)          for i < len
 * where every product and every sum is rounded to fp32 on its own, left to right, and the first product is not added to a zero:
 * the bits of a host loop of float32 products and sums in entry order.  So one entry of weight 1.0f copies a row bit for bit
 * (a NaN's payload aside).  A row may be named more than once.  A clip whose entry range is empty, whose offsets lie outside
 * [0, n_entries] or decrease, or one of whose idx[e] lies outside [0, bank_rows) gets quiet NaNs (0x7fc00000) in its len floats
 * instead, and the bank is never read outside its rows.  Every named float of dst is written exactly once and nothing else is
 * written; the bank, offsets, idx and w are read only.  Rows that start on 16-byte boundaries (bank 16-byte aligned, bank_stride
 * a multiple of 4) are read 16 bytes at a time, others float by float: the same bits.
 * MST_ERR_ARG, and nothing is launched: a null pointer; n_clips, bank_rows, n_entries or len < 1; a negative stride; dst_stride
 * < len with n_clips > 1; the ranges of the bank's rows and of the destinations intersecting or not representable; a pointer
 * not 4-byte aligned; more than 2^31 - 1 chunks of 1024 floats in all. */
int32_t mst_style_mix(const float* bank, int32_t bank_rows, int64_t bank_stride,
                      const int32_t* offsets /* DEVICE int32[n_clips + 1] */, const int32_t* idx /* DEVICE int32[n_entries] */,
                      const float* w /* DEVICE float[n_entries] */, int32_t n_entries, float* dst, int64_t dst_stride,
                      int32_t n_clips, int64_t len, mst_stream stream);

/* mst_info_decide: apply_style's decisions, per clip, from the predictions of the info stage.  Clip k's predictions are the
 * n_logits floats at instruments_pred + k * pred_stride, the 2 at mode_pred + k * pred_stride and the 1 at bpm_pred + k *
 * pred_stride; its results go to instr / mode / bpm + k * out_stride (a batched plan's slots: both strides are its clip stride).
 *   ranking  the logits in descending order; equal logits by ascending index; a NaN after every number, NaNs by index.
 *   picks    percussion is index n_logits - 1; pick c < channels is the c-th entry of the ranking that is not percussion.
 *   instr    channels rows of (n_logits - 1) + n_groups floats: one_hot(pick c, n_logits - 1) ++ one_hot(group_of[pick c],
 *            n_groups) — style.data.encode_instruments of the picked programs.  group_of: HOST memory, n_logits - 1 int32 in
 *            [0, n_groups), read at the call.
 *   mode     the one-hot (2 floats) of the first index of the larger mode logit (index 0 when they are equal or unordered).
 *   bpm      rintf(bpm_pred): halves go to even.
 *   record   decisions[k * (channels + 2) ...]: the picks, percussion's position in the ranking, the mode index.
 * pool != 0: the logits, the mode logits and bpm_pred are first summed over the clips 0 ... n - 1, each an fp32 left-to-right
 * sum in clip order that starts from clip 0's value, n = *live clamped to [1, n_clips] (live: one DEVICE int32, NULL = n_clips);
 * bpm is that sum divided by n.  The one decision is written to every clip, so that all windows of one file play the same
 * instruments.  Every float of the three results of every clip and every word of decisions is written exactly once and nothing
 * else is written; the predictions are read only.
 * MST_ERR_ARG, and nothing is launched: a null pointer (live excepted); n_clips < 1; n_logits outside [2,
 * MST_DECIDE_MAX_LOGITS]; n_groups outside [1, 127]; channels outside [1, n_logits - 1]; a group_of[i] outside [0, n_groups); a
 * negative stride; out_stride < channels * (n_logits - 1 + n_groups) with n_clips > 1; a clip's three results intersecting its
 * predictions or one another; a pointer not 4-byte aligned. */
#define MST_DECIDE_MAX_LOGITS 64
int32_t mst_info_decide(const float* instruments_pred, const float* mode_pred, const float* bpm_pred, int64_t pred_stride,
                        int32_t n_logits, const int32_t* group_of /* HOST, n_logits - 1 */, int32_t n_groups, int32_t channels,
                        int32_t n_clips, int32_t pool, const int32_t* live /* DEVICE, one int32, or NULL = all */,
                        float* instr, float* mode, float* bpm, int64_t out_stride,
                        int32_t* decisions /* n_clips x (channels + 2) */, mst_stream stream);

/* ---- style search: which rows of a bank resemble a style.  The cosines of n_queries queries (len floats each, query_stride
 * floats apart) against the rows of a bank (bank_rows runs of len floats, bank_stride floats apart) and, per query, the k best
 * rows.  No reference counterpart: the reference keeps no library of styles.  Two launches — scores and the k best of every slab
 * of MST_SEARCH_SLAB rows, then a merge per query — both enqueue-only on `stream` (no allocation, no host synchronisation,
 * capturable as a single chain), without atomics and without a workgroup waiting for another: the same bits on every run.  Every
 * index array is DEVICE memory, read on the device: a captured call serves other queries, another n_live and other groups.
 *
 * Arithmetic, for query q and row r:
 *   dot(q, r)   acc = +0.0f; for i = 0 ... len - 1 in ascending order: acc = fmaf(q[i], r[i], acc).  One fp32 chain per pair,
 *               no k-split: what a k-ordered sequence of v_mfma_f32_16x16x4_f32 gives, bit for bit.
 *   nq, nr      dot(q, q) and dot(r, r), the same chain.
 *   score       dot(q, r) / (sqrtf(nq) * sqrtf(nr)): two correctly rounded roots, their product and the quotient, each rounded
 *               to fp32 on its own.
 * The score of a pair depends on the len floats of q and of r only: not on where the row sits in the bank, on which slab or
 * query tile it falls in, nor on n_queries, bank_rows or k.
 *
 * Ranking.  Row r is RANKABLE for query q when r < min(*n_live, bank_rows) (n_live: one DEVICE int32, NULL = bank_rows, a
 * negative value counts as 0); and, where groups, exclude and exclude[q] >= 0 are all given, groups[r] != exclude[q]; and the
 * score is not NaN (a zero row or a zero query gives 0 / 0 and drops out by itself).  The rankable rows are ordered by
 * order * score descending (order = +1: the nearest first, -1: the farthest first), compared as floats, equal keys by ascending
 * row; rows[q * k + j] and scores[q * k + j] hold the j-th of that order, positions past the last rankable row hold row -1 and
 * score 0x7fc00000.  So `rows` can be handed to mst_style_mix as its idx, with offsets[q] = q * k.  Every word of rows and
 * scores is written exactly once and nothing else is written, scratch aside (mst_style_search_scratch_bytes(bank_rows,
 * n_queries, k) bytes, 8-byte aligned; <= 0 on arguments mst_style_search refuses); the bank, groups, queries and exclude are
 * read only.  Rows that start on 16-byte boundaries (bank 16-byte aligned, bank_stride a multiple of 4; the queries likewise)
 * are read 16 bytes per lane, others float by float: the same bits.  Rows at and behind bank_rows are never read; a slab
 * wholly behind *n_live is not read either.
 * MST_ERR_ARG, and nothing is launched: a null bank, queries, rows, scores or scratch; bank_rows, n_queries or len < 1;
 * n_queries > 4096; len > 4096; k outside [1, MST_SEARCH_MAX_K]; order not +1 or -1; a negative stride; a float or int pointer
 * not 4-byte aligned; scratch not 8-byte aligned; rows / scores intersecting each other, the bank's rows or the queries, or these
 * ranges not representable; exclude given without groups; more than 2^31 - 1 workgroups (slabs x tiles of 64 queries). */
#define MST_SEARCH_MAX_K 16
#define MST_SEARCH_SLAB 64
int64_t mst_style_search_scratch_bytes(int32_t bank_rows, int32_t n_queries, int32_t k);
int32_t mst_style_search(const float* bank, int32_t bank_rows, int64_t bank_stride,
                         const int32_t* n_live /* DEVICE, one int32, or NULL = bank_rows */,
                         const int32_t* groups /* DEVICE int32[bank_rows] or NULL */,
                         const float* queries, int32_t n_queries, int64_t query_stride,
                         const int32_t* exclude /* DEVICE int32[n_queries] or NULL */,
                         int64_t len, int32_t k, int32_t order /* +1 nearest, -1 farthest */,
                         int32_t* rows /* n_queries x k */, float* scores /* n_queries x k */,
                         void* scratch, mst_stream stream);

/* ---- instrumentation (bench.py only; synchronises on HIP events, never used for training):
 * average duration of every launch step of a pass, with its algorithmic FLOPs and bytes.
 * kind: 0 gemm, 1 gather, 2 segment-reduce, 3/4 lstm fwd/bwd, 5/6 combine fwd/bwd, 7/8 melody notes, 9/10 applier notes,
 * 11 lstm weight transpose, 12/13 row-wise tiny Linear fwd/bwd, ..., 26-28 conv.hip prep / forward / weight gradient,
 * 29-31 lin.hip forward / input gradient / weight gradient. */
int32_t mst_plan_step_count(const mst_plan* p, int32_t stage_mask, int32_t backward);
int32_t mst_plan_step_info(const mst_plan* p, int32_t stage_mask, int32_t backward, int32_t* info /* 8 ints per step: 4 shape values, member count, kind, dependency level (inside its chain), chain (-1 = none) */);
/* One int per step of the pass (the steps mst_plan_step_info lists): 0 = the step is launched on its own; 1 = the step, a gather
 * or a segment reduce, has no launch of its own: it is carried by the GEMM step of its dependency level, whose gemm_kernel grid runs
 * its workgroups in front of the GEMM members' (one-stream, merged plans on the 32x32 tiling only); 2 = a carried two-stage segment
 * reduce: its first stage rides, its second stage stays a launch, directly behind the GEMM launch.  mst_plan_launch_count counts
 * a carried step's first stage as 0 launches.  mst_plan_time_steps times the GEMM step together with everything it carries and
 * reports a carried step as a row of 0 ms with its own FLOPs / bytes.  Always 0 for LSTM steps, carried or not (and every kind but
 * gathers and segment reduces): mst_plan_step_carrier reports those.  Returns the step count. */
int32_t mst_plan_step_carried(const mst_plan* p, int32_t stage_mask, int32_t backward, int32_t* carried);
/* The same for every step kind a GEMM launch can carry (gathers, segment reduces, and the combine steps of plans with at most 4
 * channels): 0 = own launch(es); 1 = the whole step is in its level's GEMM launch (a gather, a one-stage segment reduce, a small
 * combine site); 2 = the first stage is carried and the second stage is a launch directly behind the carrier (a two-stage segment
 * reduce, a large combine).  mst_plan_step_carried keeps reporting gathers and segment reduces only.  Always 0 for LSTM steps,
 * carried or not: mst_plan_step_carrier reports those.  Returns the step count. */
int32_t mst_plan_step_riders(const mst_plan* p, int32_t stage_mask, int32_t backward, int32_t* out);
/* 1 = mst_train_iteration clears the whole-model zero list (mst_zero_grads' ranges, with the LSTM exchange tags) inside its first
 * forward launch: that launch is a GEMM step of a plan that carries riders, and the plan proved that nothing the launch reads or
 * writes overlaps a zero chunk.  0 = the zero list is a launch of its own, as in mst_zero_grads. */
int32_t mst_plan_zero_rides(const mst_plan* p);
/* One int per step of the pass: the index, within the same list, of the step whose launch runs it (the GEMM step of its level that
 * carries it: every carried kind), or -1 for a step with a launch of its own.  Besides gathers, segment reduces and combines
 * that is a backward LSTM step whose hidden sizes are all <= 8 and that would not take the grouped flavour, on a level with a
 * GEMM step (of its own stage where stages run separately): one wave of a gemm_kernel rider block runs one sequence.  Forward
 * LSTM steps and larger hidden sizes keep their launch.  Returns the step count. */
int32_t mst_plan_step_carrier(const mst_plan* p, int32_t stage_mask, int32_t backward, int32_t* out);
/* The LSTM launches of a plan whose hidden sizes are all <= 16 (and that do not take the grouped flavour of batched plans) run on
 * the one-wave kernels: one wave per sequence, no workgroup barrier.  on = 0 makes them use the register-flavour kernels of
 * H <= 64 instead (bit-identical results; for tests and profiling); on = 1 is the default.  MST_ERR_UNSUPPORTED on a plan in
 * which a GEMM launch carries an LSTM step (mst_plan_step_carrier): meant for no_merge = 1 plans. */
int32_t mst_plan_set_lstm_small(mst_plan* p, int32_t on);
/* (new) instrumentation: the members of GEMM launch step `step` of a pass, one clip's worth, 6 values each:
 * {M, N, K, k-splits, folded rows per clip (0 = not folded), workgroups}.  Returns the member count (<= cap). */
int32_t mst_plan_step_gemms(const mst_plan* p, int32_t stage_mask, int32_t backward, int32_t step, int32_t* out, int32_t cap);
int32_t mst_plan_time_steps(const mst_plan* p, int32_t stage_mask, int32_t backward, const float* params,
                            float* gparams, float* ws, const float* pitched, const float* unpitched,
                            mst_stream stream, int32_t reps, float* ms, int32_t* kind, double* flops, double* bytes);

/* ---- AUDIO EXTENSION — NOT REFERENCE PARITY.  The reference has no audio path (latex/music-style-transfer.tex:79-80 names it as
 * future work; requirements.txt:1-8 has no audio library); BASELINE.json's metric text nevertheless speaks of 30 s @ 44.1 kHz clips,
 * an STFT(1024/256) featuriser and a feature-Gram style loss, and SURVEY.md 8(f4) keeps that as an optional extension with a
 * build-defined oracle (oracle/audio_oracle.py: torch.stft / matmul / autograd on the CPU; parity unpinned).  Nothing of the hot
 * path above uses these entry points.
 * Layout: a clip of n_samples mono float samples -> frames = 1 + n_samples / hop frames (centre-padded by reflection, periodic Hann
 * window: torch.stft's defaults) x bins = n_fft / 2 + 1; magnitude / feature matrices are (frames x ld) row-major with
 * ld = bins rounded up to a multiple of 8 and zero pad columns; Gram matrices are (ld x ld), pads zero. */
typedef struct mst_audio_plan mst_audio_plan;
mst_audio_plan* mst_audio_plan_create(int32_t n_fft /* 1024 | 2048 */, int32_t hop, int64_t n_samples, int32_t* status);
void mst_audio_plan_destroy(mst_audio_plan* p);
/* out = {frames, bins, ld, workspace floats of mst_audio_gram / mst_audio_style_iteration, k-splits of the Gram, Gram tiles} */
int32_t mst_audio_plan_info(const mst_audio_plan* p, int64_t out[6]);
/* spec: frames x bins complex64 (re, im interleaved) or NULL; mag: frames x ld or NULL (at least one) */
int32_t mst_audio_stft(const mst_audio_plan* p, const float* audio, float* spec, float* mag, mst_stream stream);
/* gram = feat^T feat / frames (ld x ld) on the f32 matrix cores; ws: workspace (mst_audio_plan_info) */
int32_t mst_audio_gram(const mst_audio_plan* p, const float* feat, float* gram, float* ws, mst_stream stream);
/* One optimisation iteration on x (frames x ld): loss = || x^T x / frames - gram_style ||_F^2 (written to *loss, a device float),
 * grad = (4 / frames) x (x^T x / frames - gram_style) (written to `grad`, frames x ld), then Adam(lr, .9, .999, 1e-8) on x with
 * state tensors exp_avg / exp_avg_sq (frames x ld) and `state` (4 floats, as mst_adam_step). */
int32_t mst_audio_style_iteration(const mst_audio_plan* p, float* x, const float* gram_style, float* grad, float* exp_avg,
                                  float* exp_avg_sq, float* state, float* ws, float* loss, double lr, mst_stream stream);

/* test hook of the plan builder's single-launch weight-gradient reduction guard: do two column blocks of one row-major matrix
 * (row pitch ld), given by their first elements' offsets from the matrix's element (0, 0), share no element?  1 = disjoint. */
int32_t mst_debug_slab_columns_disjoint(int64_t off_x, int32_t width_x, int64_t off_y, int32_t width_y, int32_t ld);
/* test hook of the 32x32 GEMM kernel's tile loaders: walks a whole operand on the host with the per-lane walk state the kernel
 * uses (every lane of every 32-row tile, k-tiles of depth kd = 32 | 64 | 128 over [k0, k1), k0 a multiple of 8, k1 <= K) and
 * compares each element's predicates and offset with the closed-form accessor.  kind: 3 im2col (as A: lanes walk k, `rows` = M;
 * as_b = 1: lanes walk the column, `rows` = N), 4 permuted weight (as_b = 1; (pb, pc) = (14, 5) or (47, 2), row pitch ld),
 * 5 conv gradient (as A, oc out channels).  Returns the number of mismatching elements (0 = the walk is the accessor), or a
 * negative MST_ERR_*; *compared (nullable) receives the number of elements walked. */
int64_t mst_debug_gemm_walk(int32_t kind, int32_t as_b, int32_t rows, int32_t K, int32_t k0, int32_t k1, int32_t kd, int32_t ld,
                            int32_t pb, int32_t pc, int32_t oc, int64_t* compared);
/* the members of GEMM launch step `step` (as mst_plan_step_gemms, same order), 2 values each: {kernel variant (GV_* of the
 * plan's tiling), k-tile depth (32 | 64 | 128 on the 32x32 tiling, 32 on the 64x64 tiling)}.  Returns the member count (<= cap). */
int32_t mst_plan_step_gemm_kinds(const mst_plan* p, int32_t stage_mask, int32_t backward, int32_t step, int32_t* out, int32_t cap);

const char* mst_version(void);

#ifdef __cplusplus
}
#endif
#endif
