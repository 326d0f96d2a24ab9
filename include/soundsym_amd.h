/*
 * soundsym_amd.h -- C ABI of the MI355X-native segment-distance matcher.
 *
 * This is the drop-in boundary for ONE hot path of andrewcsmith/soundsym: the all-pairs
 * segment-distance search + per-target argmin.  The reference has no FFI of its own (pure Rust,
 * no `extern "C"`); every entry point below names the reference interface it replaces so that a
 * maintainer can bind it 1:1 from Rust (`INTEGRATION.md` shows the binding).  Reference citations
 * are relative to the upstream repository root.
 *
 * Conventions
 *   - plain C: opaque handles, plain pointers and sizes, no C++ types, no exceptions;
 *   - every function returns an int32 status (0 = SSYM_OK, negative = error); the message for the
 *     last failure on a context is ssym_last_error(ctx);
 *   - a "segment" is what the reference calls a Sound inside a SoundDictionary / SoundSequence:
 *     `frames x dim` feature values, frame-major, contiguous (Sound::mfccs(), src/sound.rs:189-193;
 *     segment slicing src/sound.rs:330-343).  A set of segments is handed over as ONE flat value
 *     buffer plus `n+1` FRAME offsets: segment i = values [off[i]*dim, off[i+1]*dim);
 *   - the library COPIES caller memory at create time (the caller keeps ownership, like the Rust
 *     side keeps its Vec<Arc<Sound>>); results are indices into the dictionary, the Rust side
 *     then does `dict.sounds[idx].clone()` exactly as src/sound.rs:369 does;
 *   - calls are synchronous on the caller's thread, like the reference (no threads there).  One
 *     context per thread, or an external lock.  A context owns one HIP stream on one GPU;
 *   - there is NO CPU fallback: without a usable gfx950 device ssym_ctx_create fails with
 *     SSYM_E_NO_DEVICE.
 *
 * Metric modes (SURVEY.md section 0 / DESIGN.md)
 *   SSYM_METRIC_REFCOS  the reference's own segment distance: cosine_sim (src/sound.rs:22-33,
 *                       prefix dot / product of squared norms, f64) searched by at_distance
 *                       (src/sound.rs:351-370): argmin_i |sim_i - distance|, first minimum wins,
 *                       fold start (0, 2.0).  Arithmetic order follows the reference bit for bit.
 *   SSYM_METRIC_DTW     dynamic time warping over frame-wise L2 local costs with min-of-three
 *                       recurrence and optional Sakoe-Chiba band (not in the reference; defined
 *                       in DESIGN.md).  argmin_i |cost_i - distance| (distance NULL = 0), first
 *                       minimum wins, fold start (0, +inf).
 */
#ifndef SOUNDSYM_AMD_H
#define SOUNDSYM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSYM_ABI_VERSION 3

#if defined(__GNUC__)
#define SSYM_API __attribute__((visibility("default")))
#else
#define SSYM_API
#endif

typedef struct ssym_ctx ssym_ctx;         /* one GPU + one stream + scratch                      */
typedef struct ssym_dict ssym_dict;       /* SoundDictionary's feature side (src/sound.rs:290)   */
typedef struct ssym_queries ssym_queries; /* the targets of one batch (SoundSequence::sounds)    */
typedef struct ssym_samples ssym_samples; /* the dictionary sounds' SAMPLES, resident on the GPU   */
typedef struct ssym_comm ssym_comm;       /* one rank of a source-sharded run: an RCCL communicator  */
typedef struct ssym_gmm ssym_gmm;         /* a trained Gaussian mixture (the partitioner's model)    */
typedef struct ssym_stream ssym_stream;   /* growing sounds: samples + analysis resident on the GPU  */
typedef struct ssym_spotter ssym_spotter; /* targets watched in growing sources: resumable spotting   */
typedef struct ssym_coverer ssym_coverer; /* growing targets tiled by dictionary segments: live cover  */
typedef struct ssym_mosaicker ssym_mosaicker; /* growing targets tiled by free spans: live mosaic       */
typedef struct ssym_resynth ssym_resynth; /* committed mosaic frames to audio, push by push: live resynthesis */
typedef struct ssym_follower ssym_follower; /* loudness tracking, push by push: live envelope following */

enum {
    SSYM_OK = 0,
    SSYM_E_INVALID = -1,     /* bad argument (NULL, dim mismatch, non-monotonic offsets, ...)    */
    SSYM_E_EMPTY_DICT = -2,  /* replaces the reference's panic at src/sound.rs:369               */
    SSYM_E_NO_DEVICE = -3,   /* no usable gfx950 device / HIP runtime -- there is no CPU path    */
    SSYM_E_HIP = -4,         /* a HIP call failed; see ssym_last_error                           */
    SSYM_E_NOMEM = -5,
    SSYM_E_UNSUPPORTED = -6, /* shape outside what the kernels handle (see DESIGN.md limits)     */
    SSYM_E_TIMEOUT = -7,     /* ssym_match_sharded: a rank did not arrive within the communicator's
                                deadline; the communicator has been ABORTED (ncclCommAbort) and can
                                only be destroyed                                                */
    SSYM_E_COMM = -8         /* the communicator is dead (aborted by an earlier failure on this or
                                another rank, or RCCL reported an asynchronous error)            */
};

enum { SSYM_METRIC_REFCOS = 0, SSYM_METRIC_DTW = 1 };
enum { SSYM_DTYPE_F64 = 0, SSYM_DTYPE_F32 = 1 };

/* flags for ssym_match_queries */
enum {
    SSYM_OUT_DEVICE = 1u,      /* out_idx / out_cost are device pointers on ctx's GPU            */
    SSYM_DTW_FORCE_EXACT = 2u, /* skip the f32 MFMA filter: exact f64 kernel on every pair       */
    SSYM_DTW_PRUNE = 4u        /* dtw first-minimum search (k = 1, no per-target distances): one
                                  candidate pair per target is scored first and the filter
                                  abandons pairs that are provably above it; same indices and
                                  costs, the time then depends on the data; ignored where it does
                                  not apply                                                       */
};

typedef struct ssym_config {
    uint32_t struct_size;  /* = sizeof(ssym_config)                                              */
    int32_t device;        /* HIP device ordinal                                                 */
    int32_t metric;        /* SSYM_METRIC_*                                                      */
    int32_t dtype;         /* SSYM_DTYPE_* of every feature buffer handed to this context        */
    int32_t band;          /* dtw: Sakoe-Chiba radius in frames, -1 = none                       */
    int32_t dtw_squared;   /* dtw: 0 = L2 local cost (default), 1 = squared L2                   */
    void *stream;          /* hipStream_t to enqueue on; NULL = the library creates one          */
    int32_t dtw_prune;     /* dtw: 1 = every batched match of at least 64 targets runs as if          */
                           /* SSYM_DTW_PRUNE were passed (the entry points without a flags argument,  */
                           /* ssym_match_batch, included); 0 = only where the flag is given           */
    int32_t reserved;      /* 0                                                                  */
} ssym_config;

/* Per-phase device time of the LAST ssym_match_* (or ssym_dtw_spot / ssym_spot_queries) call on the context, measured
 * with HIP events recorded on the context's stream (milliseconds; 0 when a phase did not run).  One exception: a refcos search
 * through a filter (refcos_filter 1 or 2) outside ssym_match_sharded is timed by the device's wall clock, read by
 * its first kernel, the first kernel after the main one and its last kernel -- an event record between two kernels
 * costs several microseconds of gap on the stream, which a search of 0.2 ms notices. */
typedef struct ssym_timings {
    float pack_ms;      /* target packing (only when the call packed targets itself)             */
    float main_ms;      /* dtw: MFMA filter kernel / refcos: similarity tile kernel              */
    float select_ms;    /* dtw: bounds, two-stage candidate selection, certificates              */
    float refine_ms;    /* dtw: exact f64 re-scoring of candidates (or of every pair)            */
    float reduce_ms;    /* final per-target argmin                                               */
    float total_ms;     /* first event to last event                                             */
    uint64_t n_pairs;   /* n_sources * n_targets of the call                                     */
    uint64_t n_refined; /* dtw: pairs re-scored exactly                                          */
    int32_t main_launches; /* kernel launches that made up main_ms                               */
    int32_t used_filter;   /* dtw: 1 = MFMA filter + refine, 0 = exact kernel on every pair      */
    float prune_ms;        /* SSYM_DTW_PRUNE: candidate search + exact scores + thresholds        */
    int32_t pruned;        /* 1 = the filter ran with early abandoning                           */
    uint64_t n_filter_cells; /* dtw, unbanded filter: DP cells it evaluated, padding included (pruned runs: counted by
                                the kernel; full runs: from the launches' geometry); 0 elsewhere   */
    float collective_ms;   /* ssym_match_sharded: the RCCL all-reduce(s) + all-gather, device time  */
    int32_t attempts;      /* ssym_match_sharded: selection attempts of the step (1 unless a rank's
                              candidate list overflowed and every rank redid the tail)             */
    int32_t exact_redone;  /* dtw: launches of the exact kernel whose wave-pipelined variant gave up
                              waiting and whose list was scored again by the plain variant (0 in any
                              healthy run; results are correct either way)                          */
    int32_t refcos_filter; /* refcos searches: 0 = the exact tile kernel on every pair, 1 = the f64 matrix-pipe
                              filter, 2 = the integer (i8 matrix-pipe) filter; exact keys on the candidates
                              either way (this word was `reserved` before: same size and place)        */
} ssym_timings;

SSYM_API int32_t ssym_abi_version(void);

/* Context ------------------------------------------------------------------------------------ */
SSYM_API int32_t ssym_ctx_create(const ssym_config *cfg, ssym_ctx **out);
SSYM_API int32_t ssym_ctx_destroy(ssym_ctx *ctx);
SSYM_API const char *ssym_last_error(const ssym_ctx *ctx); /* ctx may be NULL: last create failure       */
SSYM_API int32_t ssym_ctx_synchronize(ssym_ctx *ctx);
SSYM_API int32_t ssym_get_timings(const ssym_ctx *ctx, ssym_timings *out);

/* Dictionary: replaces SoundDictionary::{new, from_segments, add_segments}
 * (src/sound.rs:296, 323, 330) as far as features are concerned.
 *   feats          flat values, dtype per cfg.dtype (HOST memory)
 *   frame_offsets  n_segments + 1 offsets in FRAMES, non-decreasing, frame_offsets[0] may be > 0
 *   dim            values per frame (NCOEFFS = 12 in the reference, src/lib.rs:22)
 * n_segments = 0 creates an empty dictionary (SoundDictionary::new); matching against it fails
 * with SSYM_E_EMPTY_DICT. */
SSYM_API int32_t ssym_dict_create(ssym_ctx *ctx, const void *feats, const uint64_t *frame_offsets,
                         uint32_t n_segments, uint32_t dim, ssym_dict **out);
/* Same, but `feats` is a DEVICE pointer on the context's GPU (offsets stay on the host). */
SSYM_API int32_t ssym_dict_create_device(ssym_ctx *ctx, const void *feats_dev,
                                const uint64_t *frame_offsets, uint32_t n_segments, uint32_t dim,
                                ssym_dict **out);
/* add_segments (src/sound.rs:330): appended segments get the next indices. */
SSYM_API int32_t ssym_dict_append(ssym_ctx *ctx, ssym_dict *dict, const void *feats,
                         const uint64_t *frame_offsets, uint32_t n_segments);
SSYM_API int32_t ssym_dict_size(const ssym_dict *dict, uint32_t *out_n_segments);
SSYM_API int32_t ssym_dict_destroy(ssym_ctx *ctx, ssym_dict *dict);

/* Targets of one batch, made resident once (the `for sound in self.sounds` side of
 * clone_from_dictionary, src/sound.rs:453). */
SSYM_API int32_t ssym_queries_create(ssym_ctx *ctx, const void *feats, const uint64_t *frame_offsets,
                            uint32_t n_targets, uint32_t dim, ssym_queries **out);
SSYM_API int32_t ssym_queries_create_device(ssym_ctx *ctx, const void *feats_dev,
                                   const uint64_t *frame_offsets, uint32_t n_targets,
                                   uint32_t dim, ssym_queries **out);
SSYM_API int32_t ssym_queries_destroy(ssym_ctx *ctx, ssym_queries *q);

/* The hot path.  Replaces the loop of clone_from_dictionary (src/sound.rs:451-455: one
 * match_sound per target) and of morph_to (src/sound.rs:440-446: one at_distance per target).
 *   distance    NULL: 1.0 per target in refcos (match_sound, src/sound.rs:346-348), 0.0 in dtw;
 *               else n_targets values in HOST memory (morph_to's distances)
 *   index_base  added to every returned index (a rank holding the source shard [base, base+n)
 *               returns global indices)
 *   out_idx     n_targets u32: chosen dictionary index per target (+ index_base)
 *   out_cost    nullable, n_targets f64: refcos -> the winning |sim - distance| (the reference's
 *               discarded `min_distance`, src/sound.rs:361-368); dtw -> the winner's DTW cost.
 *               When nothing beats the fold start the index is 0 (+ index_base) and the value is
 *               the fold start (2.0 / +inf), as in src/sound.rs:361-367.  A target whose `distance` entry is NaN
 *               or infinite is such a target on either metric: every key is NaN or +inf and none is below the
 *               fold start, so it gets index 0 (+ index_base) and 2.0 / +inf.  So is a refcos target whose
 *               distance lies 2.0 or more from every similarity (1e301, say).
 *   flags       SSYM_OUT_DEVICE, SSYM_DTW_FORCE_EXACT
 * Returns after the results are written (the stream is synchronised). */
SSYM_API int32_t ssym_match_queries(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                           const double *distance, uint32_t index_base, uint32_t *out_idx,
                           double *out_cost, uint32_t flags);

/* The k best dictionary entries per target ("top-k candidates"; the
 * reference itself only ever takes the first: at_distance, src/sound.rs:351-370).  Same inputs as
 * ssym_match_queries; entry r of target t is at [t * k + r].  Entries are ordered by
 * (|value - distance|, index) ascending, value = cosine_sim in refcos, DTW cost in dtw -- so entry 0
 * is ssym_match_queries' answer whenever anything beats the fold start (key < 2.0 in refcos,
 * finite cost in dtw; NaN keys never enter, as in src/sound.rs:362).  When fewer than k entries
 * qualify the rest of the row is SSYM_NO_MATCH with cost NaN.  out_cost as in ssym_match_queries
 * (refcos: the key |sim - distance|; dtw: the cost).  1 <= k <= SSYM_TOPK_MAX.  dtw results are
 * those of an exact f64 evaluation of every pair, as for k = 1.
 * index_base is added to the entries that name a dictionary entry and to nothing else: a missing entry is
 * SSYM_NO_MATCH itself whatever the base.  A NaN or infinite `distance` entry leaves nothing below the fold start
 * for its target, so for k > 1 the whole row is SSYM_NO_MATCH / NaN.  k = 1 IS ssym_match_queries, outputs
 * included: such a target then has index 0 + index_base and the fold start, not a missing entry.  Equal keys from
 * either side of a distance (sim_1 - d = d - sim_2) are ordered by index like any other tie. */
#define SSYM_TOPK_MAX 64u
#define SSYM_NO_MATCH 0xffffffffu
SSYM_API int32_t ssym_match_topk(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                        const double *distance, uint32_t k, uint32_t index_base, uint32_t *out_idx,
                        double *out_cost, uint32_t flags);

/* Convenience: pack host targets, match, release.  Same contract as ssym_match_queries with
 * host outputs. */
SSYM_API int32_t ssym_match_batch(ssym_ctx *ctx, const ssym_dict *dict, const void *tgt_feats,
                         const uint64_t *tgt_frame_offsets, uint32_t n_targets,
                         const double *distance, uint32_t *out_idx, double *out_cost);

/* One query: SoundDictionary::at_distance(distance, other) (src/sound.rs:351) /
 * match_sound(other) (src/sound.rs:346, pass distance = 1.0 in refcos). */
SSYM_API int32_t ssym_match_one(ssym_ctx *ctx, const ssym_dict *dict, const void *feats,
                       uint64_t n_frames, double distance, uint32_t *out_idx, double *out_cost);

/* SoundSequence::from_distances (src/sound.rs:405-417): starting from `start`, step i matches the
 * previous step's result (the start sound for i = 0) with at_distance(distances[i], .) and the
 * match becomes the next query.  out_idx[i] / out_cost[i] (nullable) are step i's result, as
 * ssym_match_one would return them.  The chain runs on the device without a host round trip per
 * step: in refcos the later steps are row lookups in the dictionary's self-similarity matrix,
 * which is computed on first use and kept with the dictionary (hence the non-const handle;
 * n^2 f64 of device memory) until ssym_dict_append changes it; in dtw every step re-scores the
 * dictionary against the current entry with the exact f64 kernel.
 * A step at which no key is below the fold's start (2.0 in refcos, +inf in dtw: zero-norm, NaN or empty entries only,
 * a distance that far away, no pair inside the band) reports index 0 and the fold's start, and the chain goes on
 * from entry 0 as the reference's fold does (src/sound.rs:361-369).  n_steps = 0 succeeds and does nothing; one step
 * does not build the matrix.  NULL dict / distances / out_idx, or NULL start_feats with start_frames > 0:
 * SSYM_E_INVALID; an empty dictionary: SSYM_E_EMPTY_DICT; the outputs are unwritten then. */
SSYM_API int32_t ssym_chain(ssym_ctx *ctx, ssym_dict *dict, const void *start_feats, uint64_t start_frames,
                   const double *distances, uint32_t n_steps, uint32_t *out_idx, double *out_cost);

/* The whole [n_sources][n_targets] matrix in HOST memory, row-major, f64:
 *   refcos: cosine_sim(source, target) (src/sound.rs:22-33), bit for bit (exact = 0 or 1); exact = 2 -> the
 *           similarities the f64 matrix pipe's dots give (the filter of the refcos search: FMA chains in another
 *           summation order, within (3 L + 16) 2^-53 sqrt(norm(me) norm(you)) / nrm of the reference's);
 *           exact = 3 -> the similarities of the integer filter (the refcos search's default filter: every value as a
 *           23-bit fixed-point number per segment, exact integer products; SSYM_E_UNSUPPORTED where that filter does
 *           not take the sets, e.g. values that are not finite);
 *   dtw:    exact = 0 -> the f32 MFMA filter's costs (frames wider than 42 values: of their first 42
 *           values only; a Sakoe-Chiba band beyond the banded kernel, r > 47: the unbanded cost --
 *           either way a lower bound of every pair's cost); exact = 1 -> the exact f64 costs. */
SSYM_API int32_t ssym_pair_matrix(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                         int32_t exact, double *out_matrix);

/* DTW alignment (dtw contexts only; DESIGN.md section 2 "Alignment" and section 5.12): for a list of (source, target)
 * pairs the optimal warping path of the context's recurrence (its band and cost mode), the path's cost and a map from
 * target frames onto source frames, in one call.  The reference has no counterpart: it never warps.
 *   Pair p = (dictionary segment src_idx[p] - index_base, target tgt_idx[p]); tgt_idx == NULL: target p (n_pairs <=
 *   n_targets), so ssym_match_queries' out_idx can be passed straight in.  Any pairing, repeats allowed.  src_idx[p] ==
 *   SSYM_NO_MATCH: no path, cost +inf.  src_idx / tgt_idx / offsets are HOST memory.
 *   Path: cells (i, j), i = source frame, j = target frame, from (0, 0) to (Fa - 1, Fb - 1), every step one of (+1,+1),
 *   (+1,0), (0,+1); max(Fa, Fb) <= L <= Fa + Fb - 1 cells.  Found backwards from the end cell on the exact f64 D: at
 *   (i, j), with dg = D(i-1,j-1), up = D(i-1,j), lf = D(i,j-1) (outside the matrix or the band: +inf), go diagonally if
 *   dg <= up && dg <= lf, else up (i - 1) if up <= lf, else left (j - 1).
 *   out_cost   n_pairs f64: D(Fa-1, Fb-1), the bits ssym_pair_matrix(exact = 1) returns for the pair
 *   out_len    n_pairs u32: L, or 0 when the cost is not finite (an empty segment, a band that cuts every path, NaN
 *              features, SSYM_NO_MATCH): then neither the path slot nor the map slot of the pair is written.  A pair
 *              with a feature that is not finite has the exact kernel's cost, ssym_pair_matrix(exact = 1)'s: +inf or
 *              NaN, never finite (every path crosses the poisoned row or column)
 *   out_path   2 u32 (i, j) per cell, forward order, pair p from cell index path_offsets[p] on
 *   out_map    nullable; u32 per target frame, pair p from map_offsets[p] on: map[j] = the smallest i with (i, j) on the
 *              path (non-decreasing, map[0] = 0)
 *   flags      SSYM_OUT_DEVICE: out_cost, out_len, out_path and out_map are device memory
 * ssym_dtw_align_sizes (host arithmetic, no device work) fills both offset arrays (n_pairs + 1 u64 each, starting at 0)
 * with the room a pair can need: Fa + Fb - 1 cells and Fb map entries, 0 for SSYM_NO_MATCH or an empty segment.
 * ssym_dtw_align accepts any non-decreasing offsets that leave at least that room per pair.
 * Limits: every listed segment at most 4096 frames, dim <= 64; beyond them, and on a refcos context,
 * SSYM_E_UNSUPPORTED.  NULL pointers, an index outside its set, a dim mismatch, decreasing or too small offsets:
 * SSYM_E_INVALID; an empty dictionary with n_pairs > 0: SSYM_E_EMPTY_DICT -- all with a message, before device memory
 * is touched and with the outputs unwritten.  n_pairs = 0 succeeds and does nothing.  One synchronisation per call. */
SSYM_API int32_t ssym_dtw_align_sizes(const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                      const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base,
                                      uint64_t *path_offsets, uint64_t *map_offsets);
SSYM_API int32_t ssym_dtw_align(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, double *out_cost,
                                uint32_t *out_len, const uint64_t *path_offsets, uint32_t *out_path,
                                const uint64_t *map_offsets, uint32_t *out_map, uint32_t flags);

/* DTW spotting (subsequence DTW; dtw contexts without a band; DESIGN.md section 2 "Spotting" and section 5.15): where
 * inside an unsegmented dictionary recording a target aligns best.  The source side of the recurrence is open at both
 * ends; the reference has no counterpart.  With c the context's local cost (its squared option applies), i a source
 * frame 0 ... Fa - 1, j a target frame 0 ... Fb - 1:
 *   D(i,0)  = c(i,0)                                    for every i (a path may start at any source frame)
 *   D(i,j)  = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)),  j >= 1, outside the matrix +inf
 *   st(i,0) = i;  st(i,j) = st of the predecessor ssym_dtw_align's rule picks: with dg = D(i-1,j-1), up = D(i-1,j),
 *             lf = D(i,j-1): diagonal if dg <= up && dg <= lf, else up if up <= lf, else left
 *   end     = the smallest i at which D(i,Fb-1) is least (i ascending from (none, +inf), strict <: NaN never wins)
 *   cost    = D(end,Fb-1);  start = st(end,Fb-1)
 * in the arithmetic of ssym_pair_matrix(exact = 1) and ssym_dtw_align (f64, k ascending, every operation rounded
 * separately).  So start is where ssym_dtw_align's backtrace from (end, Fb-1) first reaches column 0, cost has the bits
 * of the plain DTW cost of (source frames start ... end, target) -- what ssym_pair_matrix(exact = 1) and ssym_dtw_align
 * give for that cut -- and is the least such cost over all spans.  The cost is NOT normalised by any length.
 * Features that are not finite: min compares from D(i-1,j), then D(i,j-1), then D(i-1,j-1), strict <, so a NaN source
 * frame makes every later end a non-candidate for a target of two or more frames (D(i-1,j) carries the NaN down every
 * column j >= 1; column 0 restarts, so a one-frame target loses that row alone), and a NaN target frame makes every
 * end NaN or +inf: no spot.  +-inf and a value whose squared difference overflows cost +inf in their own row, and the
 * rows behind it spot again.  Neither NaN nor +inf wins; no read leaves its buffer.
 * ssym_dtw_spot: pair p = (dictionary segment src_idx[p] - index_base, target tgt_idx[p]); tgt_idx == NULL: target p
 *   (n_pairs <= n_targets).  Any pairing, repeats allowed.  src_idx / tgt_idx are HOST memory.
 *   out_cost   n_pairs f64;  out_start, out_end   n_pairs u32 each: the span's first and last source frame (inclusive)
 *   No spot (src_idx[p] == SSYM_NO_MATCH, a segment without frames, no finite D(i,Fb-1)): cost +inf, start = end =
 *   SSYM_NO_MATCH.
 *   flags      SSYM_OUT_DEVICE: out_cost, out_start and out_end are device memory
 * ssym_spot_queries: every dictionary segment against every target, then per target the first least cost over ascending
 *   segment index (strict < from (SSYM_NO_MATCH, +inf)): out_idx n_targets u32 (+ index_base; SSYM_NO_MATCH itself when
 *   no segment has a spot), out_cost / out_start / out_end those of that segment.  n_sources * n_targets < 2^32.
 *   flags      SSYM_OUT_DEVICE: the four outputs are device memory
 * Limits: targets of at most 4096 frames, dim <= 64; beyond them, on a refcos context and on a context with a band (a
 * Sakoe-Chiba band has no meaning with a free start): SSYM_E_UNSUPPORTED.  A source may be as long as a dictionary
 * segment can be: ssym_dict_create takes segments of up to 2^31 - 1 frames.  NULL pointers, an index outside its set, a
 * dim mismatch: SSYM_E_INVALID; an empty dictionary with work to do (n_pairs > 0, n_targets > 0): SSYM_E_EMPTY_DICT --
 * all with a message, before device memory is touched and with the outputs unwritten.  n_pairs = 0 / n_targets = 0
 * succeeds and does nothing.  One synchronisation per call.  ssym_get_timings afterwards: main_ms = the spot kernel,
 * reduce_ms = the fold of ssym_spot_queries, n_pairs = the pairs of the call. */
SSYM_API int32_t ssym_dtw_spot(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                               const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, double *out_cost,
                               uint32_t *out_start, uint32_t *out_end, uint32_t flags);
SSYM_API int32_t ssym_spot_queries(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t index_base,
                                   uint32_t *out_idx, double *out_cost, uint32_t *out_start, uint32_t *out_end,
                                   uint32_t flags);

/* Occurrences (DESIGN.md section 2 "Occurrences" and section 5.16): up to K pairwise disjoint spans per (source, target)
 * pair, best first -- every place a target sounds inside a recording, not only the best one.  c, D, st, the squared
 * option and the arithmetic are those of ssym_dtw_spot above.  For one pair with Fa, Fb >= 1:
 *   delta(i) = D(i,Fb-1),  s(i) = st(i,Fb-1)            for i = 0 ... Fa - 1 (the end-column profile)
 *   candidate: an end i with delta(i) finite and delta(i) <= max_cost (+inf when max_cost is NULL), not yet dead
 *   pick m   : the candidate with the least delta, among equals the smallest i (i ascending from (none, +inf), strict <)
 *              -> occurrence m = (cost delta(i*), start s(i*), end i*)
 *   kill     : every end i with s(i) <= i* and i >= s(i*) is dead from now on (its span [s(i), i] shares a frame with
 *              [s(i*), i*]; i* itself is among them)
 *   stop     : after K picks, or when no candidate is left
 *   count    = picks made;  slots count ... K - 1 hold (+inf, SSYM_NO_MATCH, SSYM_NO_MATCH)
 *   nothing  : Fa = 0, Fb = 0, source SSYM_NO_MATCH -> count 0
 * So, without max_cost, occurrence 0 is ssym_dtw_spot's result for the pair bit for bit; costs do not decrease with m and
 * equal costs come in ascending end; spans are pairwise disjoint in frames (touching, end_a + 1 = start_b, is allowed);
 * every occurrence's cost has the bits of the plain DTW cost of (source frames start ... end, target), what
 * ssym_pair_matrix(exact = 1) gives for that cut; a NaN delta(i) is never a candidate.  As for ssym_dtw_spot, a NaN
 * source frame makes every later end a non-candidate for a target of two or more frames, so occurrences behind it are
 * not found, and a NaN target frame makes every end NaN or +inf: count 0.  The cost is NOT normalised by any
 * length: without max_cost the later occurrences of a recording that holds the target fewer than K times are spans the
 * target merely fits least badly.
 * ssym_dtw_spot_all: the pair list is ssym_dtw_spot's in every respect (tgt_idx == NULL, repeats, index_base,
 *   SSYM_NO_MATCH sources, HOST memory).
 *   max_spots  K, 1 ... 64
 *   max_cost   HOST memory, n_pairs f64, one threshold per pair; NULL: none
 *   out_count  n_pairs u32;  out_cost  n_pairs * K f64;  out_start, out_end  n_pairs * K u32 each, row-major [n_pairs][K]
 *   flags      SSYM_OUT_DEVICE: the four outputs are device memory
 * Limits: those of ssym_dtw_spot (targets of at most 4096 frames, dim <= 64, no band, no refcos), and every listed
 * source at most 2^24 = 16777216 frames (the profile lives in device scratch at 12 bytes per source frame; a call's scratch
 * stays within 512 MiB): beyond them SSYM_E_UNSUPPORTED.  max_spots 0 or > 64, a NaN in max_cost, NULL pointers, an index
 * outside its set, a dim mismatch: SSYM_E_INVALID; an empty dictionary with n_pairs > 0: SSYM_E_EMPTY_DICT -- all with a
 * message, before device memory is touched and with the outputs unwritten.  n_pairs = 0 succeeds and does nothing
 * (max_spots, max_cost and the outputs are not looked at then).  One synchronisation per call.  ssym_get_timings afterwards: main_ms = the kernel (forward pass and selection are one
 * launch), n_pairs = the pairs of the call. */
SSYM_API int32_t ssym_dtw_spot_all(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                   const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t max_spots,
                                   const double *max_cost, uint32_t *out_count, double *out_cost, uint32_t *out_start,
                                   uint32_t *out_end, uint32_t flags);

/* Paced spotting (DESIGN.md section 2 "Paced spotting" and section 5.18): the three calls above with a step pattern.
 * SSYM_STEP_SYMMETRIC is the recurrence of ssym_dtw_spot: the _step calls are then the calls above, bit for bit.
 * SSYM_STEP_PACED is the asymmetric pattern with Itakura's rule: every target frame takes exactly one source frame; a
 * source frame may be skipped, but never two in a row; a source frame may be repeated, but never twice in a row.  Every
 * admissible path has exactly Fb cells, so cost / Fb is a mean per-frame distance that compares across targets of
 * different lengths, and every span has between floor((Fb-1)/2) + 1 and 2 Fb - 1 frames.  c, the squared option and the
 * arithmetic are those of ssym_dtw_spot (f64, k ascending, every operation rounded separately).  Every cell has two
 * states, N (entered by a source step) and H (entered by repeating the source frame):
 *   N(i,0) = c(i,0), sN(i,0) = i;   H(i,0) = +inf (no start)
 *   E(i,j) = the cell's better state: (N, sN); if H(i,j) < N(i,j): (H, sH)        (strict <: a tie keeps N)
 *   j >= 1:
 *     P      = E(i-1,j-1); if E(i-2,j-1) < P: E(i-2,j-1)   (strict <: a tie keeps the diagonal; outside the matrix +inf)
 *     N(i,j) = c(i,j) + P.value,      sN(i,j) = P.start
 *     H(i,j) = c(i,j) + N(i,j-1),     sH(i,j) = sN(i,j-1)  (a repeat may only follow a source step)
 *   delta(i) = E(i,Fb-1).value,  s(i) = E(i,Fb-1).start    (the end-column profile)
 *   end  = the smallest i at which delta(i) is least (i ascending from (none, +inf), strict <: NaN and +inf never win)
 *   cost = delta(end),  start = s(end);  no spot (Fa = 0, Fb = 0, SSYM_NO_MATCH, no finite delta): (+inf, SSYM_NO_MATCH,
 *   SSYM_NO_MATCH)
 * So cost is the least sum of c over all admissible paths of every start and end, summed in path order (acc = c + acc),
 * and end the first end that reaches it.  A target equal to every second frame of a stretch of the source costs exactly
 * 0.0 with a span of 2 Fb - 1 frames; one equal to a stretch with each frame doubled costs 0.0 with a span of Fb / 2
 * frames; the same stretch with each frame tripled costs more than 0, where ssym_dtw_spot gives 0.0.  Features that are
 * not finite: the strict < comparisons above decide; a span with a NaN or +inf cost is never reported and no read
 * leaves its buffer.  Occurrences under the paced pattern (ssym_dtw_spot_all_step) use this delta and s; candidates,
 * picks, kills, the stop, max_cost, the count and the padding are those of "Occurrences" above, word for word.
 * Costs stay unnormalised sums, and max_cost is a sum: the caller forms per-frame values (cost / Fb, max_cost = x * Fb).
 * Pair lists, SSYM_NO_MATCH, tgt_idx == NULL, flags, the error codes, outputs unwritten on refusal, n_pairs = 0 and the
 * timings are those of the three calls above.  An unknown step: SSYM_E_INVALID.
 * Limits with SSYM_STEP_PACED: targets of at most 2048 frames (two hand-off rows take 24 bytes of LDS per target frame),
 * dim <= 64, sources as long as a dictionary segment; ssym_dtw_spot_all_step keeps the 2^24 source frames and the
 * 512 MiB of scratch of ssym_dtw_spot_all.  A longer target, a refcos context, a context with a band:
 * SSYM_E_UNSUPPORTED before any device work. */
#define SSYM_STEP_SYMMETRIC 0u
#define SSYM_STEP_PACED 1u
SSYM_API int32_t ssym_dtw_spot_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                    const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t step,
                                    double *out_cost, uint32_t *out_start, uint32_t *out_end, uint32_t flags);
SSYM_API int32_t ssym_spot_queries_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t index_base,
                                        uint32_t step, uint32_t *out_idx, double *out_cost, uint32_t *out_start,
                                        uint32_t *out_end, uint32_t flags);
SSYM_API int32_t ssym_dtw_spot_all_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                                        const uint32_t *src_idx, const uint32_t *tgt_idx, uint32_t n_pairs,
                                        uint32_t index_base, uint32_t step, uint32_t max_spots, const double *max_cost,
                                        uint32_t *out_count, double *out_cost, uint32_t *out_start, uint32_t *out_end,
                                        uint32_t flags);

/* Paced alignment (DESIGN.md section 2 "Paced alignment" and section 5.19): ssym_dtw_align with a step pattern.
 * SSYM_STEP_SYMMETRIC is ssym_dtw_align itself: one host path, the same kernel, the same bits.  SSYM_STEP_PACED is the path
 * of the paced pattern above between pinned ends -- the alignment that goes with a paced spot: cut the span out of the
 * recording, align it with the target under the same pattern, warp along the map.  c, the squared option and the
 * arithmetic are those of "Paced spotting" (f64, k ascending, every sub, mul, add and sqrt rounded separately, no
 * contraction); i is a source frame 0 ... Fa - 1, j a target frame 0 ... Fb - 1:
 *   shape   : Fa = 0, Fb = 0, SSYM_NO_MATCH, or Fa outside floor((Fb-1)/2) + 1 ... 2 Fb - 1  ->  cost +inf, L = 0, decided
 *             before the recurrence
 *   N(0,0) = c(0,0);  N(i,0) = +inf for i >= 1;  H(i,0) = +inf
 *   E(i,j) = N(i,j); if H(i,j) < N(i,j): H(i,j)                       (strict <: a tie keeps N)
 *   j >= 1:  P = E(i-1,j-1); if E(i-2,j-1) < P: E(i-2,j-1)             (strict <; outside the matrix = +inf)
 *            N(i,j) = c(i,j) + P;   H(i,j) = c(i,j) + N(i,j-1)
 *   cost    = E(Fa-1,Fb-1);  L = Fb if the cost is finite, else 0 (no path, no map, slots unwritten)
 *   backward: at (Fa-1,Fb-1) the state is H if H < N there, else N.
 *             state H at (i,j): the cell before is (i, j-1), in state N.
 *             state N at (i,j): the cell before is (i-2,j-1) if E(i-2,j-1) < E(i-1,j-1), else (i-1,j-1); its state is H
 *             if H < N there, else N.
 *   path[j] = (i_j, j);  map[j] = i_j
 * So map[0] = 0 and map[Fb-1] = Fa - 1, every map[j+1] - map[j] is 0, 1 or 2 and never 0 twice in a row; acc = c(p_0),
 * acc = c(p_j) + acc along the path reproduces cost bit for bit; cost is the least such sum over all admissible pinned
 * paths; and for a span [start, end] that ssym_dtw_spot_step or ssym_dtw_spot_all_step reports under SSYM_STEP_PACED, the
 * cost of (source frames start ... end, target) has that spot's cost bits.  Path and map are the same thing here (one
 * source frame per target frame), and the map is what ssym_reconstruct_warped and ssym_reconstruct_wsola take.  Features
 * that are not finite: the strict < comparisons above decide over the whole matrix.  A value that is not finite in a
 * target frame or in the first or last source frame is on every path, and a NaN in any source frame spreads down the
 * diagonals: the cost is NaN or +inf and L = 0.  A source frame in between whose local costs are +inf is stepped over
 * where the pattern allows a skip, as paced spotting finds spans behind such a frame.  No read leaves its buffer.
 * Parameters, pair lists, SSYM_NO_MATCH, flags, error codes, n_pairs = 0 and outputs unwritten on refusal are
 * ssym_dtw_align's.  A paced pair needs room for Fb cells and Fb map entries; ssym_dtw_align_sizes leaves at least that.
 * An unknown step: SSYM_E_INVALID.  Limits with SSYM_STEP_PACED: targets of at most 2048 frames (two hand-off rows take 16
 * bytes of LDS per target frame), sources of at most 4096 frames, dim <= 64; beyond them, on a refcos context and on a
 * context with a band (the pattern bounds the slope itself): SSYM_E_UNSUPPORTED before any device work. */
SSYM_API int32_t ssym_dtw_align_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                     const uint32_t *tgt_idx, uint32_t n_pairs, uint32_t index_base, uint32_t step,
                                     double *out_cost, uint32_t *out_len, const uint64_t *path_offsets, uint32_t *out_path,
                                     const uint64_t *map_offsets, uint32_t *out_map, uint32_t flags);

/* Span alignment (DESIGN.md section 2 "Spans" and section 5.22): ssym_dtw_align and ssym_dtw_align_step with a span of
 * source frames per pair, so that what ssym_dtw_spot, ssym_dtw_spot_all and their _step forms report is aligned where it
 * lies, in the resident dictionary, without cutting the recording.
 *   span_first, span_last   n_pairs u32 each (HOST): inclusive source frames inside segment src_idx[p] - index_base
 *   step                    SSYM_STEP_SYMMETRIC or SSYM_STEP_PACED
 * Definition by reduction: pair p gives exactly what the existing call gives for the pair (S', target), S' a dictionary
 * segment that holds frames span_first[p] ... span_last[p] of that segment -- with SSYM_STEP_SYMMETRIC ssym_dtw_align
 * (the context's band and squared option included), with SSYM_STEP_PACED ssym_dtw_align_step(SSYM_STEP_PACED).  out_cost,
 * out_len, the path and the map are those bits; the NaN and +-inf rules and the tie rules are those; the paced shape rule is
 * applied to Fa' = last - first + 1.  Path cells and out_map are RELATIVE TO THE SPAN: map[0] = 0, and source frame
 * first + map[j] of the recording goes with target frame j, so the map feeds ssym_reconstruct_warped_spans and
 * ssym_reconstruct_wsola_spans unchanged.  ssym_dtw_align_spans_sizes leaves Fa' + Fb - 1 cells and Fb map entries per
 * pair.  span_first[p] == span_last[p] == SSYM_NO_MATCH -- what a spot without a span returns -- is "no path", like
 * src_idx[p] == SSYM_NO_MATCH: cost +inf, out_len 0, slots unwritten (nothing else of the pair's span is looked at when
 * src_idx[p] is SSYM_NO_MATCH).  Frames outside the span are never read.
 * Errors: first > last, last >= the segment's frames, exactly one of the two SSYM_NO_MATCH, a NULL span array with
 * n_pairs > 0: SSYM_E_INVALID; every error case of the existing calls keeps its code.  Limits hold for the SPAN, not the
 * segment: Fa' <= 4096, targets <= 4096 frames (<= 2048 under SSYM_STEP_PACED), dim <= 64, dtw contexts only, no band under
 * SSYM_STEP_PACED, fewer than 2^31 pairs; beyond them SSYM_E_UNSUPPORTED.  The segment itself may be as long as a
 * dictionary holds.  Every error comes with a message, before any device work, with the outputs unwritten.
 * SSYM_OUT_DEVICE, n_pairs = 0, the one synchronisation per call and ssym_get_timings are ssym_dtw_align's. */
SSYM_API int32_t ssym_dtw_align_spans_sizes(const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                            const uint32_t *tgt_idx, const uint32_t *span_first, const uint32_t *span_last,
                                            uint32_t n_pairs, uint32_t index_base, uint64_t *path_offsets,
                                            uint64_t *map_offsets);
SSYM_API int32_t ssym_dtw_align_spans(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const uint32_t *src_idx,
                                      const uint32_t *tgt_idx, const uint32_t *span_first, const uint32_t *span_last,
                                      uint32_t n_pairs, uint32_t index_base, uint32_t step, double *out_cost,
                                      uint32_t *out_len, const uint64_t *path_offsets, uint32_t *out_path,
                                      const uint64_t *map_offsets, uint32_t *out_map, uint32_t flags);

/* Paced matching (DESIGN.md section 2 "Paced matching" and section 5.21): ssym_match_queries and ssym_pair_matrix with a
 * step pattern.  SSYM_STEP_SYMMETRIC makes them the existing calls: one host path, the same kernels, the same bits
 * (ssym_pair_matrix_step is then ssym_pair_matrix with exact = 1).  Under SSYM_STEP_PACED, for source s (Fa frames) and
 * target t (Fb frames), cost(s, t) is EXACTLY the cost of "Paced alignment" above: the shape rule decided before the
 * recurrence (Fa = 0, Fb = 0 or Fa outside floor((Fb-1)/2) + 1 ... 2 Fb - 1 gives +inf), column 0 pinned at source frame 0,
 * the states N, H, E, P with their strict < comparisons, the same arithmetic (f64, k ascending, every sub, mul, add and
 * sqrt rounded separately, no contraction) over the whole matrix, the context's squared option.  So a matrix entry has the
 * bits ssym_dtw_align_step(SSYM_STEP_PACED) returns in out_cost for that pair, and is not finite exactly where that is not.
 * Per target the result follows ssym_match_queries' dtw rule: idx[t] = argmin_s |cost(s,t) - distance[t]| (distance NULL
 * = 0), the first minimum wins, the fold starts at (0, +inf), a NaN or +inf key never wins, out_cost (nullable) is the
 * winner's cost, and a target nothing beats gets 0 + index_base and +inf.  Whenever out_cost[t] is finite,
 * ssym_dtw_align_step(SSYM_STEP_PACED) on (out_idx[t], t) gives out_len = Fb and that cost, bit for bit.  Every admissible
 * path has Fb cells, so cost / Fb is a true mean per frame; costs stay sums here and the caller divides.  Neither cost
 * bounds the other (a paced step that skips a source frame is no symmetric step), so no filter runs in front: every
 * shape-feasible pair is evaluated in f64, and SSYM_DTW_FORCE_EXACT and SSYM_DTW_PRUNE mean nothing under SSYM_STEP_PACED
 * and are ignored there.  SSYM_OUT_DEVICE is honoured.  index_base is honoured, so the results of dictionary shards go
 * through ssym_merge_shards as they are.  out_matrix: [n_sources][n_targets] f64, HOST memory.
 * Limits with SSYM_STEP_PACED: a dtw context without a band, dim <= 64, every target of at most 2048 and every source of at
 * most 4096 frames (ssym_dtw_align_step's, so every reported match can be aligned); beyond them and on a refcos context:
 * SSYM_E_UNSUPPORTED before any device work, with the outputs unwritten.  An unknown step: SSYM_E_INVALID.  An empty
 * dictionary: SSYM_E_EMPTY_DICT.  n_targets = 0 succeeds and does nothing.  One synchronisation per call.
 * ssym_get_timings afterwards: main_ms = the forward kernel, reduce_ms = the fold, n_pairs = n_sources x n_targets. */
SSYM_API int32_t ssym_match_queries_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, const double *distance,
                                         uint32_t index_base, uint32_t step, uint32_t *out_idx, double *out_cost,
                                         uint32_t flags);
SSYM_API int32_t ssym_pair_matrix_step(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, uint32_t step,
                                       double *out_matrix);

/* Cover (DESIGN.md section 2 "Cover" and section 5.23): every target tiled by dictionary segments, the cut points and the
 * segments chosen together so that the paced costs of the pieces sum to the least total over every tiling.  Under the paced
 * pattern every tiling of a T-frame target has exactly T cells, so totals compare and total / T is a mean per frame.
 * For one target X of T frames and sources n = 0 ... N-1 of Fa[n] frames, in the arithmetic of "Paced alignment" above:
 *   w(n,s,L)  = cost(n, X[s ... s+L-1]) of "Paced matching": +inf where the shape rule says no, else E(Fa-1, L-1); a source of
 *               Fa frames covers windows of ceil((Fa+1)/2) ... 2 Fa frames only
 *   M(s,L)    = the first least w(n,s,L) over n ascending from (none, +inf), strict < (NaN and +inf never win) -> src(s,L)
 *   best(-1)  = 0
 *   best(e)   = scan L = 1 ... min(e+1, 2 Fmax) ascending from (none, +inf), strict <, over the L that have a src(e-L+1, L):
 *               v = (M(e-L+1, L) + piece_penalty) + best(e-L)  -> the first least v, its (L, src, M)
 *   cover     : walk back from e = T-1 while best is finite: piece (src, start = e-L+1, end = e, cost = M); e <- e-L
 *   total     = best(T-1); count = pieces, reported in ascending start;  no cover (T = 0, best(T-1) not finite): count 0,
 *               total +inf
 * So the pieces tile [0, T); a piece's cost has the bits ssym_pair_matrix_step and ssym_dtw_align_step give under
 * SSYM_STEP_PACED for (src, the cut X[start ... end]); acc = 0, acc = (cost_k + piece_penalty) + acc in piece order gives
 * total's bits; total is the least such sum; on a tie the lower source index wins, then the shorter last piece.  A NaN or
 * +-inf in a target frame: no cover.  A dictionary segment with a NaN frame is never chosen.  No read leaves its buffer.
 *   piece_penalty  >= 0, finite: added per piece, trades total fit for fewer, longer pieces; 0 is the plain optimum
 *   out_count, out_total   n_targets u32 / f64
 *   out_src, out_start, out_end, out_cost   one slot per target frame of the whole query set; target t's pieces start at
 *               slot frame_offset[t] (a cover never has more pieces than frames); unused slots hold (SSYM_NO_MATCH,
 *               SSYM_NO_MATCH, SSYM_NO_MATCH, +inf).  start / end count frames inside the target.  Costs are sums.
 *   flags       SSYM_OUT_DEVICE: the six outputs are device memory
 * The targets of one call are independent covers.
 * Limits: a dtw context without a band, dim <= 64, every dictionary segment of at most 128 frames (kCoverMaxSourceFrames),
 * and scratch of frames x 2 Fmax x 12 + frames x 16 bytes <= 512 MiB (frames: the target frames of the call, Fmax: the
 * longest dictionary segment; the M / src tables of one source block and the back-pointers).  Beyond them and on a refcos
 * context: SSYM_E_UNSUPPORTED before any device work, with the outputs unwritten.  A NaN, negative or infinite
 * piece_penalty: SSYM_E_INVALID.  An empty dictionary: SSYM_E_EMPTY_DICT.  n_targets = 0 succeeds and does nothing.  One
 * synchronisation per call.  ssym_get_timings afterwards: main_ms = the forward pass (with its fold), reduce_ms = the chain,
 * n_pairs = n_sources x the call's target frames. */
SSYM_API int32_t ssym_dtw_cover(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty,
                                uint32_t flags, uint32_t *out_count, double *out_total, uint32_t *out_src,
                                uint32_t *out_start, uint32_t *out_end, double *out_cost);

/* Cover with gaps (DESIGN.md section 2 "Cover with gaps" and section 5.23): the cover, with target frames left uncovered at
 * gap_cost per frame.  Everything of "Cover" above holds word for word: c, w, M, src, the scan over L, best(-1) = 0.  One
 * candidate is added to each step:
 *   best(e)   : the scan of "Cover" gives (v, L, src, M) or (+inf, none)
 *               vg = gap_cost + best(e-1)
 *               if vg < v (strict):  best(e) = vg, back-pointer (L = 1, src = SSYM_COVER_GAP, M = gap_cost)
 *   cover     : walk back as before; a gap frame is the piece (SSYM_COVER_GAP, start = e, end = e, cost = gap_cost)
 *   total     : acc = 0; a piece: acc = (cost + piece_penalty) + acc; a gap frame: acc = gap_cost + acc  -> total's bits
 * A gap is reported FRAME BY FRAME, one slot each (so a cover still never has more pieces than frames); piece_penalty is not
 * charged on a gap frame; a piece wins a tie against a gap.  So: (1) the pieces and gap frames tile [0, T); (2) a piece's
 * cost is still the paced alignment's for the cut, bit for bit; (3) the re-summation above gives total; (4) total is the
 * least such sum over every tiling with gaps; (5) with a finite gap_cost every target of T >= 1 frames has a cover: a NaN or
 * +-inf target frame is a gap frame, and the frames on both sides of it are covered; (6) gap_cost = +inf never wins: the six
 * outputs are ssym_dtw_cover's, bit for bit; (7) no read leaves its buffer.
 *   gap_cost    >= 0 and finite, or +inf: the price per frame, comparable with a piece's cost per frame
 * Outputs, flags, limits, refusals, scratch and timings are ssym_dtw_cover's.  A NaN, negative or -inf gap_cost:
 * SSYM_E_INVALID before any device work, with the outputs unwritten. */
#define SSYM_COVER_GAP 0xFFFFFFFEu
SSYM_API int32_t ssym_dtw_cover_gaps(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty,
                                     double gap_cost, uint32_t flags, uint32_t *out_count, double *out_total,
                                     uint32_t *out_src, uint32_t *out_start, uint32_t *out_end, double *out_cost);

/* Mosaic (DESIGN.md section 2 "Mosaic" and section 5.25): every target tiled by pieces, each piece ANY span of ANY dictionary
 * segment aligned under the paced pattern; the cuts, the segments, the spans and the paths are chosen together.  Neither
 * side needs cutting beforehand: the dictionary may be whole recordings of any length.  Under the paced pattern every
 * tiling of a T-frame target has exactly T cells, so totals compare and total / T is a mean per frame.
 * c, the squared option and the arithmetic are those of "Paced spotting" above, word for word.  The dictionary's segments
 * are laid end to end: g = 0 ... G-1 is a global source frame, seg(g) its segment, pos(g) its frame within it; empty
 * segments contribute nothing.  Every cell has the states N and H of the paced pattern.  For one target X of T frames:
 *   best(-1) = 0
 *   column j = 0 ... T-1:
 *     S      = piece_penalty + best(j-1)                            (the price of opening a piece at column j)
 *     P(g)   = E(g-1, j-1) if pos(g) >= 1, else +inf
 *              if pos(g) >= 2 and E(g-2, j-1) < P: E(g-2, j-1)       (strict <; j = 0: P = +inf)
 *     open(g)= not (P(g) <= S)                                      (a tie continues the piece; a NaN P opens)
 *     Q      = S if open(g) else P(g)
 *     H(g,j) = c(g,j) + N(g,j-1)                                    (+inf at j = 0; a repeat may only follow a source step)
 *     N(g,j) = c(g,j) + Q
 *     E(g,j) = N(g,j); if H(g,j) < N(g,j): H(g,j)                   (strict <: a tie keeps N)
 *     (v,arg)= the first least E(g,j) over g ascending from (+inf, none), strict <   (NaN and +inf never win)
 *     vg     = gap_cost + best(j-1);  if vg < v (strict): best(j) = vg, arg(j) = GAP;  else best(j) = v, arg(j) = arg
 *   total    = best(T-1);  no mosaic: T = 0, or total not finite -> count 0, total +inf
 *   backward : j = T-1, at arg(j).  GAP: frame j is a gap frame, go to arg(j-1).  Otherwise the state is H if H < N there,
 *              else N.  State H at (g,j): the cell before is (g, j-1) in state N.  State N at (g,j): if open(g) at column
 *              j, a piece starts here, go to arg(j-1); else the cell before is (g-2, j-1) if the P rule took it, else
 *              (g-1, j-1), in its E state.
 * So (1) pieces and gap frames tile [0, T); within a piece the source frame advances by 0, 1 or 2 per target frame, never
 * by 0 twice in a row, and a piece never crosses a segment boundary; (2) acc = 0; a frame that opens a piece: acc = c +
 * (piece_penalty + acc); one that continues a piece: acc = c + acc; a gap frame: acc = gap_cost + acc -> total's bits;
 * (3) total is the least such sum over every mosaic; (4) a NaN source frame is never on a path; a NaN target frame means
 * no mosaic without gaps and exactly one gap frame with a finite gap_cost; (5) no read leaves its buffer.  At
 * piece_penalty = 0 the optimum is frame-wise and a stretched span comes back in fragments: ask with a penalty > 0.
 *   piece_penalty  >= 0, finite: charged once per piece, never on a gap frame
 *   gap_cost       >= 0 and finite, or +inf (no gaps): the price of a target frame left uncovered
 *   out_count, out_total   n_targets u32 / f64: pieces + gap frames, and total
 *   out_start      one slot per target frame of the whole query set, target t's from slot frame_offset[t]: the target
 *                  frames at which a piece or a gap frame starts, ascending; unused slots hold SSYM_NO_MATCH
 *   out_src, out_frame, out_frame_cost   per target frame: the segment, the frame within it and c; a gap frame:
 *                  (SSYM_COVER_GAP, SSYM_NO_MATCH, gap_cost); without a mosaic (SSYM_NO_MATCH, SSYM_NO_MATCH, +inf)
 *   flags          SSYM_OUT_DEVICE: the outputs are device memory.  Every output may be NULL.
 * The targets of one call are independent mosaics.
 * Limits: a dtw context without a band, dim <= 64, and for the call's longest target G x T + 32 G + 4 T + 8 bytes (one
 * workgroup's direction bytes, two columns of state and column picks) + G + 8 G dim bytes (pos and the transposed frames,
 * once per call) of scratch <= 512 MiB, G the dictionary's frames; a call with more targets than fit runs them in rounds
 * on fewer workgroups.  Segments may be as long as a
 * dictionary holds.  Beyond the limits and on a refcos context: SSYM_E_UNSUPPORTED before any device work, with the
 * outputs unwritten.  A NaN, negative or infinite piece_penalty, a NaN, negative or -inf gap_cost: SSYM_E_INVALID.  An
 * empty dictionary: SSYM_E_EMPTY_DICT.  n_targets = 0 succeeds and does nothing.  One synchronisation per call.
 * ssym_get_timings afterwards: main_ms = the forward and back-trace kernels, main_launches = the rounds, n_pairs = G x the
 * call's target frames. */
SSYM_API int32_t ssym_dtw_mosaic(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q, double piece_penalty,
                                 double gap_cost, uint32_t flags, uint32_t *out_count, double *out_total,
                                 uint32_t *out_start, uint32_t *out_src, uint32_t *out_frame, double *out_frame_cost);

/* Source-sharded multi-GPU, dtw metric: the one real exchange the path has.  Each rank's filter gives,
 * per target, an upper bound on the best key in ITS shard; a rank whose shard does not hold a
 * target's neighbour would otherwise re-score ~10^2 of its own pairs per target for nothing.
 *   ssym_match_begin   runs the filter and writes the per-target bound to bounds_dev (n_targets f64,
 *                      DEVICE memory of the caller, e.g. a torch tensor); the stream is synchronised
 *   (caller)           all-reduce(MIN) of bounds_dev over the ranks (RCCL; n_targets * 8 bytes)
 *   ssym_match_finish  selects candidates against the reduced bounds, re-scores them exactly and
 *                      writes what ssym_match_queries would (index 0 + base / +inf for a target
 *                      none of whose pairs in this shard can win -- ssym_merge_shards then takes
 *                      another shard's entry)
 * dict / q / distance must stay alive between the two calls; flags as for ssym_match_queries.
 * Any other matching call on the context in between (it would use the same scratch) ends the pair:
 * ssym_match_finish then fails with "without ssym_match_begin".
 * Where the filter does not apply (refcos, shapes outside its limits, features that are not finite, frames
 * wider than the filter's 42 values together with per-target distances) begin writes +inf and finish is a
 * plain ssym_match_queries -- for the distances and the index_base GIVEN TO BEGIN: begin keeps its own copy of
 * them, and a later begin (with other distances, or without any) replaces them.  So callers need no second
 * code path.  With one rank, or without the all-reduce, the pair is equivalent to ssym_match_queries. */
SSYM_API int32_t ssym_match_begin(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                         const double *distance, uint32_t index_base, double *bounds_dev);
SSYM_API int32_t ssym_match_finish(ssym_ctx *ctx, const double *bounds_dev, uint32_t *out_idx,
                          double *out_cost, uint32_t flags);

/* Early abandoning (SSYM_DTW_PRUNE) in a source-sharded run: only the rank that holds a target's
 * neighbour knows a tight bound before the filter, so the candidates' costs are exchanged first.
 *   ssym_match_candidates    scores this shard's candidate pair per target exactly and writes the costs
 *                            to cost_dev (n_targets f64, DEVICE memory; +inf where pruning does not
 *                            apply: refcos, frames wider than 42 values, shapes outside the filter)
 *   (caller)                 all-reduce(MIN) of cost_dev over the ranks
 *   ssym_match_begin_pruned  ssym_match_begin (no per-target distances) whose filter abandons pairs
 *                            that are provably above the reduced costs; then the all-reduce of the
 *                            bounds and ssym_match_finish as before.  Without a preceding
 *                            ssym_match_candidates on the same (dict, q) it is a plain ssym_match_begin.
 * Results are those of the unpruned sequence, bit for bit. */
SSYM_API int32_t ssym_match_candidates(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                                       double *cost_dev);
SSYM_API int32_t ssym_match_begin_pruned(ssym_ctx *ctx, const ssym_dict *dict, const ssym_queries *q,
                                         uint32_t index_base, const double *cost_dev, double *bounds_dev);

/* Source-sharded multi-GPU: after an all-gather of every shard's (cost, global index) per target
 * (n_shards x n_targets each, shard-major, DEVICE memory), pick per target the shard entry with
 * the smallest cost, lowest global index on equal cost -- the same first-minimum rule as
 * src/sound.rs:361-367 because shards are ordered by index.  Outputs are DEVICE memory.
 * As in that fold a NaN key never wins: an entry whose key is NaN loses to every entry whose key is not, whichever
 * shard holds it.  A column whose keys are ALL NaN returns shard 0's entry (index and cost) as it stands; a column of
 * +inf returns the lowest index.  n_targets = 0 succeeds and does nothing; n_shards = 0 or a NULL costs_dev / idx_dev /
 * out_idx_dev is SSYM_E_INVALID with nothing written; out_cost_dev may be NULL. */
SSYM_API int32_t ssym_merge_shards(ssym_ctx *ctx, uint32_t n_shards, uint32_t n_targets,
                          const double *costs_dev, const uint32_t *idx_dev, uint32_t *out_idx_dev,
                          double *out_cost_dev);
/* The same for matches made with per-target distances (morph_to, src/sound.rs:440-446): the shards
 * folded on |cost - distance|, so the merge does too.  `distance`: n_targets f64 in HOST memory, or
 * NULL (= ssym_merge_shards).  dtw costs only: refcos shards report the key itself, which
 * ssym_merge_shards already compares correctly.
 * Between ssym_match_begin and ssym_match_finish on the same context: a merge without distances leaves the pending
 * step alone.  A merge WITH distances uploads them to where a begin with per-target distances keeps its own for the
 * filter's finish, so it ends such a pair (ssym_match_finish then fails with "without ssym_match_begin"); it never lets
 * finish return an answer for other distances. */
SSYM_API int32_t ssym_merge_shards_at(ssym_ctx *ctx, uint32_t n_shards, uint32_t n_targets,
                             const double *costs_dev, const uint32_t *idx_dev, const double *distance,
                             uint32_t *out_idx_dev, double *out_cost_dev);

/* Source-sharded multi-GPU with the collectives INSIDE the library (RCCL over xGMI, enqueued on the context's
 * stream): the north star's "sharding the source-segment axis with an RCCL all-gather of per-target argmin
 * indices".  The reference has no counterpart -- its loop (src/sound.rs:451-455) is serial -- so these entry
 * points replace that loop for a dictionary that is split over the GPUs of one node, one process (or thread)
 * per GPU, each with its own context:
 *   ssym_comm_unique_id  rank 0 obtains the 128-byte RCCL id (ncclGetUniqueId) and hands it to the other
 *                        ranks by any means the host has (a file, a pipe, MPI, torch.distributed ...)
 *   ssym_comm_create     ncclCommInitRank on the context's device; collective over all `world` ranks
 *   ssym_match_sharded   rank g holds the dictionary shard [index_base, index_base + n) and ALL targets
 *                        (the same targets, in the same order, on every rank).  One step =
 *                          filter over the shard                      (ssym_match_begin, no host sync)
 *                          ncclAllReduce(MIN) of the M per-target bounds            (M x 8 bytes)
 *                          selection, exact re-scoring, fold                (ssym_match_finish, no host sync)
 *                          ncclAllGather of (cost f64, global index u32) per target + list status (12 M + 8 bytes)
 *                          merge: smallest key, lowest global index on ties      (ssym_merge_shards_at)
 *                        all enqueued back to back on the context's stream; the host synchronises ONCE, at the
 *                        end, and every rank returns the same, complete answer -- bit for bit what
 *                        ssym_match_queries returns for the unsharded dictionary.  Should a rank's candidate list
 *                        overflow (the gathered status says so to everyone) all ranks repeat the tail once with
 *                        the room asked for.  With SSYM_DTW_PRUNE the candidates' costs are all-reduced first
 *                        (ssym_match_candidates / ssym_match_begin_pruned).  An empty local shard takes part and
 *                        reports the fold start; a dictionary that is empty on EVERY rank is the caller's to
 *                        reject (the reference panics, src/sound.rs:369).
 *                        out_idx / out_cost / flags as for ssym_match_queries (SSYM_OUT_DEVICE honoured).
 * FAILURE on one rank is part of the protocol (the reference fails on its one thread, src/sound.rs:369,440-449; a
 * sharded replacement has to fail on ALL ranks, and may never leave a rank waiting):
 *   - a rank whose LOCAL work fails (out of memory, a HIP error, a shape the kernels reject, a C++ exception) still
 *     takes part in every collective of the step with neutral blocks and puts its status code into the block the
 *     all-gather carries anyway; after the step's one synchronisation EVERY rank returns that same code (the lowest
 *     failing rank's), ssym_last_error names the rank and the phase, and the communicator stays usable;
 *   - a rank that cannot take part at all (it cannot allocate its exchange buffers, a collective cannot be enqueued,
 *     its caller never makes the call) leaves its peers waiting: they wait under a DEADLINE (ssym_comm_set_timeout,
 *     default 60 s, $SSYM_COMM_TIMEOUT_MS), then abort their communicator (ncclCommAbort) and return
 *     SSYM_E_TIMEOUT; the rank that could not take part aborts its own and returns its error.  An aborted communicator
 *     answers every further call with SSYM_E_COMM and can only be destroyed; RCCL's asynchronous errors
 *     (ncclCommGetAsyncError) end the wait the same way.  After an abort the context's stream is drained under a
 *     second, short deadline (5 s): that ncclCommAbort makes the queued collectives leave the stream has been seen with a
 *     world-1 communicator only -- no run over more than one GPU exists, so the behaviour at world > 1 is UNVERIFIED; a
 *     stream that does not drain is reported in ssym_last_error ("did not drain"), never waited for without bound, and
 *     the context should then be destroyed.
 * RCCL is looked up at run time (symbols already in the process, else librccl.so.1 / $SSYM_RCCL_LIB), so a
 * single-GPU user needs no RCCL at all; without it the three calls fail with SSYM_E_UNSUPPORTED. */
#define SSYM_COMM_ID_BYTES 128
SSYM_API int32_t ssym_comm_unique_id(void *out_id /* SSYM_COMM_ID_BYTES */);
SSYM_API int32_t ssym_comm_create(ssym_ctx *ctx, const void *id, int32_t rank, int32_t world, ssym_comm **out);
SSYM_API int32_t ssym_comm_destroy(ssym_ctx *ctx, ssym_comm *comm);
SSYM_API int32_t ssym_match_sharded(ssym_ctx *ctx, ssym_comm *comm, const ssym_dict *dict, const ssym_queries *q,
                                    const double *distance, uint32_t index_base, uint32_t *out_idx,
                                    double *out_cost, uint32_t flags);
/* 1 when this library could bind RCCL (every symbol it calls), 0 otherwise: what the ranks of a job agree on BEFORE
 * any of them enters ssym_comm_create (a rank without RCCL would leave the others inside ncclCommInitRank). */
SSYM_API int32_t ssym_comm_available(void);
/* Deadline of one ssym_match_sharded step in milliseconds (> 0); see the failure rules above. */
SSYM_API int32_t ssym_comm_set_timeout(ssym_comm *comm, int64_t milliseconds);
/* 1 = the communicator was aborted (every call on it fails with SSYM_E_COMM), 0 = usable. */
SSYM_API int32_t ssym_comm_is_dead(const ssym_comm *comm);
/* TEST AND MEASUREMENT HOOKS.  Both refuse with SSYM_E_UNSUPPORTED unless the calling process has SSYM_TEST_HOOKS=1 in its
 * environment at the time of the call: nothing a production caller can trip over.  The same variable gates the library's
 * measurement knobs (SSYM_FILTER_*, SSYM_REFCOS_*, SSYM_EXACT_*, SSYM_CELLS_*, SSYM_PRUNE_NT: A/B switches between kernels
 * that return the same bits): without it none of them is read.  SSYM_COMM_TIMEOUT_MS and SSYM_RCCL_LIB
 * are configuration and always honoured.
 *
 * Fault injection for the containment tests (tests/test_gpu_comm.py), one shot: the NEXT ssym_match_sharded on this
 * communicator fails in `phase` (1 = the filter phase before the bound exchange, 2 = selection / re-scoring before the
 * gather).  kind 0: the local work reports SSYM_E_NOMEM (the rank takes part, every rank returns SSYM_E_NOMEM);
 * kind 1: the rank leaves the step there without its collectives (its peers meet the deadline). */
SSYM_API int32_t ssym_comm_inject_fault(ssym_comm *comm, int32_t phase, int32_t kind);
/* Replay of a larger world on one GPU (bench.py --replay-world): from now on the per-target bounds every
 * ssym_match_sharded step agrees on are the element-wise minimum of the all-reduce's result and these `n` device doubles
 * -- the bounds ssym_match_begin returns for the FULL dictionary are exactly what the ranks of a run over its shards
 * would have all-reduced -- so that a one-rank step on one shard selects and re-scores what that rank would in the
 * larger run.  The buffer stays the caller's and must outlive the steps; n = the steps' number of targets; NULL clears. */
SSYM_API int32_t ssym_comm_replay_bounds(ssym_comm *comm, const double *bounds_dev, uint32_t n);

/* The ranks of ONE process (a thread per rank, every rank its own context, on one GPU or several) without RCCL:
 * the same ssym_match_sharded, its two exchanges done with host barriers around device copies instead of
 * stream-ordered RCCL calls.  RCCL refuses two ranks on one device; this transport is how the multi-rank logic
 * (gather layout, merge over G shards, the agreed repeat after an overflow, empty shards) is exercised on a one-GPU
 * box (tests/test_gpu_comm.py).  Every rank's thread must be inside its ssym_match_sharded call at the same time. */
typedef struct ssym_local_group ssym_local_group;
SSYM_API int32_t ssym_local_group_create(int32_t world, ssym_local_group **out);
SSYM_API int32_t ssym_local_group_destroy(ssym_local_group *group);
SSYM_API int32_t ssym_comm_create_local(ssym_ctx *ctx, ssym_local_group *group, int32_t rank, ssym_comm **out);

/* Reconstruction tail (the step right after the hot path): the samples of every dictionary sound,
 * resident on the GPU (Sound::samples(), src/sound.rs:181; `sample_offsets` = n_sounds+1 SAMPLE
 * offsets into `samples`, f64, HOST memory). */
SSYM_API int32_t ssym_samples_create(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets,
                            uint32_t n_sounds, ssym_samples **out);
SSYM_API int32_t ssym_samples_destroy(ssym_ctx *ctx, ssym_samples *s);

/* clone_from_dictionary's length fit (src/sound.rs:456-465) + to_sound's concatenation (:475-480):
 * for target t the samples of dictionary sound idx[t], zero-padded or truncated to
 * out_offsets[t+1]-out_offsets[t] samples, written at out_offsets[t].
 *   idx          n_targets dictionary indices (HOST), as returned by ssym_match_*
 *   out_offsets  n_targets+1 SAMPLE offsets of the output (HOST); out_offsets[0] must be 0
 *   out_samples  nullable, out_offsets[n] f64 (HOST)
 *   out_pcm32    nullable, out_offsets[n] i32 (HOST): Sound::write_file's conversion
 *                `(i32::MAX as f64 * sample) as i32` (src/sound.rs:139; truncating, saturating,
 *                NaN -> 0)
 * Samples are copied bit for bit (-0.0 and NaN payloads included); padding is +0.0.  A target or a sound of length 0,
 * repeated indices and any n_targets are fine.  n_targets = 0, out_offsets[n] = 0 or both outputs NULL: SSYM_OK, nothing
 * written.  NULL s / idx / out_offsets, out_offsets[0] != 0, decreasing offsets, an index >= n_sounds (SSYM_NO_MATCH
 * included): SSYM_E_INVALID; a store of no sounds: SSYM_E_EMPTY_DICT -- all before device memory is touched, with the
 * outputs unwritten.  ssym_samples_create: NULL or non-zero-based or decreasing offsets, NULL samples with a non-zero
 * total: SSYM_E_INVALID and *out = NULL; n_sounds = 0 succeeds.
 * Between ssym_match_begin and ssym_match_finish on the same context: neither call keeps or disturbs anything the
 * pending step needs (ssym_reconstruct stages in scratch that finish fills afresh, ssym_samples_create allocates its
 * own), so the pair goes on and ssym_match_finish returns what the uninterrupted sequence returns, bit for bit.  */
SSYM_API int32_t ssym_reconstruct(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx,
                         const uint64_t *out_offsets, uint32_t n_targets, double *out_samples,
                         int32_t *out_pcm32);

/* Warped reconstruction (DESIGN.md section 2 "Warped reconstruction" and section 5.13): ssym_reconstruct with every
 * match resynthesised along a target-frame -> source-frame map, so that it follows the target's timing instead of being
 * cut off or padded.  The map is what ssym_dtw_align returns as out_map.  The reference has no counterpart: it never
 * warps.  Definition, with HOP = 256, BIN = 1024 and the MFCC window w[m] = 0.5 - 0.5 cos(2 pi m / 1024) (built on the
 * host with libm cos), for target t with n = out_offsets[t+1] - out_offsets[t] output samples, x[0 .. sLen) the samples of
 * dictionary sound idx[t], F = map_frames[t] and map[0 .. F) = frame_map[map_offsets[t] ..], any u32 values:
 *   Taps.  Output sample k < n has the taps j (target frames) with j * HOP <= k < j * HOP + BIN and j < F: at most four,
 *   visited in ascending j.  m = k - j * HOP; p = map[j] * HOP + m in 64-bit arithmetic; the tap is valid when p < sLen.
 *   Value.  num = sum of w[m] * x[p], den = sum of w[m] over the valid taps, both sums starting from +0.0, every product
 *   and every sum rounded separately in f64 (no contraction).  out[k] = num / den (IEEE division) when den > 0, else
 *   +0.0.  A tap whose source sample does not exist drops out of both sums, so a match does not fade where its look-ahead
 *   frames run past its own samples.  (Non-finite samples give NaN with an unspecified payload.)
 *   Fallback.  A target with F = 0, or with pair_len[t] = 0, takes ssym_reconstruct's length fit, bit for bit.
 *   out_pcm32 is ssym_reconstruct's conversion applied to out[k].
 * Plain overlap-add: repeated source frames can comb; no waveform-similarity search, no phase handling.
 *   idx, out_offsets   as for ssym_reconstruct (HOST)
 *   frame_map          u32 source frame per target frame (HOST; nullable when every map_frames[t] is 0)
 *   map_offsets        n_targets + 1 u64 (HOST): target t's map starts at frame_map[map_offsets[t]]; non-decreasing, with
 *                      map_offsets[t+1] - map_offsets[t] >= map_frames[t] (the offsets given to ssym_dtw_align)
 *   map_frames         n_targets u32 (HOST): the target's frame count (0: length fit)
 *   pair_len           nullable, n_targets u32 (HOST): ssym_dtw_align's out_len; 0 = no finite path, the length fit --
 *                      the map slot of such a pair is never read
 *   flags              SSYM_WARP_MAP_DEVICE: frame_map and pair_len are device memory, so ssym_dtw_align's device out_map
 *                      and out_len pass straight in.  No map content can cause an out-of-range read, so a device map
 *                      needs no validation.  SSYM_OUT_DEVICE: out_samples and out_pcm32 are device memory
 *   out_samples, out_pcm32   nullable, out_offsets[n] f64 / i32 (HOST, or device with SSYM_OUT_DEVICE)
 * n_targets = 0, out_offsets[n] = 0 or both outputs NULL: SSYM_OK, nothing written.  NULL s / idx / out_offsets /
 * map_offsets / map_frames, a NULL frame_map while some map_frames[t] > 0, out_offsets[0] != 0, decreasing out_offsets or
 * map_offsets, map_offsets[t+1] - map_offsets[t] < map_frames[t], an index >= n_sounds, unknown flag bits:
 * SSYM_E_INVALID; a store of no sounds: SSYM_E_EMPTY_DICT -- all with a message in ssym_last_error, before device memory
 * is touched and with the outputs unwritten.  One synchronisation per call; ssym_get_timings reports the synthesis kernel
 * alone.  The call stages in the scratch ssym_reconstruct uses, so it may run between ssym_match_begin and
 * ssym_match_finish as that call may. */
#define SSYM_WARP_MAP_DEVICE 32u
SSYM_API int32_t ssym_reconstruct_warped(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx,
                                         const uint64_t *out_offsets, uint32_t n_targets, const uint32_t *frame_map,
                                         const uint64_t *map_offsets, const uint32_t *map_frames,
                                         const uint32_t *pair_len, uint32_t flags, double *out_samples,
                                         int32_t *out_pcm32);

/* WSOLA reconstruction (DESIGN.md section 2 "WSOLA" and section 5.14): ssym_reconstruct_warped with a waveform-similarity
 * search.  Every source frame may start up to `search` samples off its nominal place map[j] * HOP, where it continues the
 * frame laid down before it best, so that a periodic source stays periodic where the map repeats or skips frames.  With
 * HOP, BIN, w[], x[0 .. sLen), F and map[0 .. F) as above and S = search, pos[j] is the sample start of source frame j:
 *   pos[0] = map[0] * HOP.  For j >= 1: nom = map[j] * HOP (64-bit); the template is the natural continuation of the frame
 *   before, tmpl[n] = x[pos[j-1] + HOP + n], n < BIN; for every lag d in -S .. S with 0 <= nom + d < sLen the candidate is
 *   cand[n] = x[nom + d + n], n < BIN (in both, a sample at or beyond sLen reads +0.0).  c(d) = sum of tmpl[n] * cand[n],
 *   e(d) = sum of cand[n] * cand[n], both sums from +0.0 in ascending n, every product and every sum rounded separately in
 *   f64; score(d) = c / sqrt(e) (IEEE division and square root), 0 when e = 0.  pos[j] = nom + d*, d* the lag of the
 *   greatest score, ties to the smaller |d|, then to the negative d.  A NaN score never wins; d* = 0 when no lag is
 *   admissible or no admissible lag has a score that is a number.
 *   Synthesis: the taps, value and out_pcm32 of ssym_reconstruct_warped with p = pos[j] + m in place of map[j] * HOP + m.
 *   Fallback: exactly that call's (F = 0 or pair_len[t] = 0: the length fit).
 * So search = 0 gives ssym_reconstruct_warped's output bit for bit, and on a diagonal map lag 0 is the template itself,
 * the greatest score by Cauchy-Schwarz.  Still no phase vocoder and no transient handling; a repeated frame is a repeated
 * frame, only laid down in phase.
 *   search             S, at most 512 samples; more: SSYM_E_INVALID before any device work
 *   out_pos            nullable, u64 per map slot laid out by map_offsets (HOST, or device with SSYM_OUT_DEVICE): pos[j]
 *                      at out_pos[map_offsets[t] + j] for j < map_frames[t] of the targets that have a path; every other
 *                      slot is left alone
 * Every other argument, the flags, the checks, the no-op cases (out_pos alone does not make work) and the errors are
 * ssym_reconstruct_warped's.  No map content and no sample content can cause an out-of-range read; a device map is not
 * validated.  One synchronisation per call.  ssym_get_timings: main_ms the search kernel, reduce_ms the synthesis kernel,
 * total_ms both.  The call stages in the scratch ssym_reconstruct uses, so it may run between ssym_match_begin and
 * ssym_match_finish as that call may. */
SSYM_API int32_t ssym_reconstruct_wsola(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx,
                                        const uint64_t *out_offsets, uint32_t n_targets, const uint32_t *frame_map,
                                        const uint64_t *map_offsets, const uint32_t *map_frames,
                                        const uint32_t *pair_len, uint32_t search, uint32_t flags, uint64_t *out_pos,
                                        double *out_samples, int32_t *out_pcm32);

/* Sample windows (DESIGN.md section 2 "Spans" and section 5.22): ssym_reconstruct_warped and ssym_reconstruct_wsola with a
 * window of samples per target, so that a spotted span is resynthesised from the resident sample store without cutting
 * the recording.
 *   win_first, win_len   n_targets u64 each (HOST), in samples
 * The two calls are the calls above with "x[0 .. sLen) = the samples of dictionary sound idx[t]" replaced by "x[0 .. sLen)
 * = samples win_first[t] ... win_first[t] + win_len[t] - 1 of sound idx[t]" (sLen = win_len[t]).  Everything else is word
 * for word the same: the taps and their validity p < sLen, WSOLA's admissible lags 0 <= nom + d < sLen, templates and
 * candidates reading +0.0 at or beyond sLen, pos[] and out_pos relative to the window, the length-fit fallback taken over
 * the window's samples, out_pcm32, the flags, the no-op cases.  So the output has the bits of the existing call on a store
 * whose sound t is that slice.  win_len[t] = 0 is allowed: the window is an empty sound.  No map content and no window
 * can cause a read outside the window, and samples outside the window never influence an output.
 * Errors: win_first[t] + win_len[t] beyond the sound's samples, a NULL window array: SSYM_E_INVALID; 2^31 targets or more:
 * SSYM_E_UNSUPPORTED; every error case of the existing calls keeps its code -- all with a message, before any device work,
 * with the outputs unwritten.  One synchronisation per call; ssym_get_timings as for the existing calls. */
SSYM_API int32_t ssym_reconstruct_warped_spans(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx,
                                               const uint64_t *win_first, const uint64_t *win_len,
                                               const uint64_t *out_offsets, uint32_t n_targets, const uint32_t *frame_map,
                                               const uint64_t *map_offsets, const uint32_t *map_frames,
                                               const uint32_t *pair_len, uint32_t flags, double *out_samples,
                                               int32_t *out_pcm32);
SSYM_API int32_t ssym_reconstruct_wsola_spans(ssym_ctx *ctx, const ssym_samples *s, const uint32_t *idx,
                                              const uint64_t *win_first, const uint64_t *win_len,
                                              const uint64_t *out_offsets, uint32_t n_targets, const uint32_t *frame_map,
                                              const uint64_t *map_offsets, const uint32_t *map_frames,
                                              const uint32_t *pair_len, uint32_t search, uint32_t flags, uint64_t *out_pos,
                                              double *out_samples, int32_t *out_pcm32);

/* Envelope following (DESIGN.md section 2 "Envelope following" and section 5.28): a post-pass that any reconstruction can go
 * through, after which it has the loudness of its target.  Every resynthesis above plays a matched span at the level it was
 * recorded at; this call scales it, hop by hop, to the level of the reference.  Definition.  For target t:
 *   - y[0..n) is the reconstruction, with n = out_offsets[t+1] - out_offsets[t].
 *   - x[0..nx) is the reference, the target's own samples, with nx = ref_offsets[t+1] - ref_offsets[t].
 *   - x[k] reads +0.0 for k >= nx.
 *   - x[k] for k >= n is never read.
 *   - w[] is the window table of mfcc_frame.hpp.
 *   - J = ceil(n / HOP).
 *   - Target t has B = J + 1 boundaries b = 0...J when n > 0, and none when n = 0.
 *
 *   energy  : E_s(b) = sum over m = 0...1023 ascending, from +0.0, of  w[m]*(s[k]*s[k]),  k = (b-2)*HOP + m,
 *             only the m with 0 <= k < n;  t = s*s; t = w[m]*t; acc = acc + t -- three roundings, no contraction
 *   gain    : g(b) = sqrt(E_x(b) / E_y(b))   (IEEE division and square root)
 *             if g(b) is NaN: g(b) = 1.0      (0/0: both silent; or a non-finite sample in a window)
 *             else if g(b) > max_gain: g(b) = max_gain     (+inf included: a silent reconstruction under a sounding target)
 *   sample  : j = k / HOP (integer), f = (k - j*HOP) / 256.0 (exact),
 *             a = g(j)*(1.0 - f);  c = g(j+1)*f;  out[k] = y[k]*(a + c)       -- each product and the sum rounded separately
 *   pcm     : out_pcm32 = ssym_reconstruct's conversion of out[k]
 *
 * The window of boundary b is centred on sample b*HOP.  It is hop-aligned.  Hop j of the output needs g(j) and g(j+1), so
 * it needs samples below (j+3)*HOP, two hops of look-ahead.  The live follower (ssym_follower_*, "Live envelope following"
 * below) releases on exactly that and is held to this call bit for bit.
 *   samples        out_offsets[n] f64: the reconstructions, packed (HOST, or device with SSYM_FOLLOW_SAMPLES_DEVICE)
 *   out_offsets    n_targets + 1 u64 (HOST): start at 0, do not decrease
 *   ref            ref_offsets[n] f64: the references, packed (HOST, or device with SSYM_FOLLOW_REF_DEVICE); may be NULL
 *                  when ref_offsets[n] = 0
 *   ref_offsets    n_targets + 1 u64 (HOST): start at 0, do not decrease
 *   max_gain       the greatest gain, finite and at least 1
 *   flags          SSYM_FOLLOW_SAMPLES_DEVICE, SSYM_FOLLOW_REF_DEVICE: that input is device memory; SSYM_OUT_DEVICE: the
 *                  three outputs are device memory
 *   out_samples    nullable, out_offsets[n] f64.  May be `samples` itself when both are device memory: the gains are
 *                  complete before any sample is rewritten
 *   out_pcm32      nullable, out_offsets[n] i32
 *   out_gain       nullable, the g(b) of all targets packed in target order, sum of B_t f64
 * No read leaves a target's own [0, n) / [0, nx): no other target's samples, and nothing of x at or beyond n, influence a
 * target's output.  A NULL ctx; unknown flag bits; a max_gain that is NaN, below 1 or infinite; NULL out_offsets or
 * ref_offsets with n_targets > 0; offsets that do not start at 0 or that decrease; NULL samples, or NULL ref with
 * ref_offsets[n] > 0, while out_offsets[n] > 0: SSYM_E_INVALID.  2^31 targets or more; a target of 2^40 samples or more;
 * more than 2^31 - 1 blocks of 32 boundaries over all targets (a target of n > 0 samples has ceil(n / 256) + 1
 * boundaries, each target's rounded up to whole blocks): SSYM_E_UNSUPPORTED.  All with a message in ssym_last_error (but for
 * the NULL ctx), before any device work and with the outputs unwritten, in this order: ctx, flags, max_gain, the number of
 * targets, NULL offsets, the offsets' start, then target by target its decrease before its length, the blocks, NULL
 * samples or ref.  Every n_targets below 2^31 is launched: the apply kernel takes the targets 65535 at a time.  n_targets = 0, out_offsets[n] = 0 or all three outputs NULL: SSYM_OK, nothing written.
 * Any context works, refcos included: nothing here aligns.  One synchronisation per call.  ssym_get_timings: main_ms the
 * gain kernel, reduce_ms the apply kernel (0 when only out_gain is asked for), total_ms both.  Host inputs are staged in
 * the scratch ssym_reconstruct uses, so the call may run between ssym_match_begin and ssym_match_finish as that call may. */
#define SSYM_FOLLOW_SAMPLES_DEVICE 64u
#define SSYM_FOLLOW_REF_DEVICE 128u
SSYM_API int32_t ssym_follow_envelope(ssym_ctx *ctx, const double *samples, const uint64_t *out_offsets, uint32_t n_targets,
                                      const double *ref, const uint64_t *ref_offsets, double max_gain, uint32_t flags,
                                      double *out_samples, int32_t *out_pcm32, double *out_gain);

/* Feature front-end, the step before the hot path: what
 * Sound::from_samples(.., None, ..) computes through analyze_mfccs (src/sound.rs:215-242) --
 * 1024-sample Hanning windows hopped by 256 (src/lib.rs:24-25), per window `n_coeffs` MFCCs between
 * f_lo and f_hi Hz (the reference: 12, 100..8000, src/sound.rs:218), frame-major.
 * PARITY UNPINNED: the reference's arithmetic is in un-vendored crates (vox_box, sample); this is a
 * self-consistent extractor whose definition is in csrc/mfcc.hip and DESIGN.md.
 *   samples      n_samples f64 (HOST)
 *   flags        SSYM_MFCC_PAD_TAIL: n_samples / 256 frames, samples past the end read as 0
 *                (default: full windows only, (n_samples - 1024) / 256 + 1);
 *                SSYM_OUT_DEVICE: out_mfccs is a device pointer (feeds ssym_*_create_device)
 *   out_mfccs    frames * n_coeffs f64, frames as ssym_mfcc_num_frames reports
 *   out_mean     nullable, n_coeffs f64 (HOST): analyze_mean_mfccs (src/sound.rs:271-286)
 * Limits: 1 <= n_coeffs <= 64, sample_rate > 0, 0 <= f_lo < min(f_hi, sample_rate / 2), else SSYM_E_INVALID;
 * f_hi above sample_rate / 2 is cut there. */
#define SSYM_MFCC_BIN 1024
#define SSYM_MFCC_HOP 256
#define SSYM_MFCC_PAD_TAIL 4u
SSYM_API int32_t ssym_mfcc_num_frames(uint64_t n_samples, uint32_t flags, uint64_t *out_frames);
SSYM_API int32_t ssym_mfcc(ssym_ctx *ctx, const double *samples, uint64_t n_samples, double sample_rate,
                  uint32_t n_coeffs, double f_lo, double f_hi, uint32_t flags, double *out_mfccs,
                  double *out_mean);
/* analyze_mfccs for a ragged batch of sounds in one call.  Sound i is
 * samples[sample_offsets[i] .. sample_offsets[i+1]); its frames are bit for bit what ssym_mfcc returns for those
 * samples with the same rate / n_coeffs / f_lo / f_hi / flags, written at out_mfccs + out_frame_offsets[i] * n_coeffs.
 *   sample_offsets     n_sounds + 1 (HOST), non-decreasing; empty sounds allowed; n_sounds = 0 is a no-op
 *   flags              SSYM_MFCC_PAD_TAIL (a window reads zeros past ITS OWN sound's end, never the next sound),
 *                      SSYM_OUT_DEVICE (out_mfccs is device memory)
 *   out_frame_offsets  nullable, n_sounds + 1 u64 (HOST): prefix sums of ssym_mfcc_num_frames per sound
 *   out_mfccs          total_frames * n_coeffs f64 (size it with ssym_mfcc_num_frames per sound)
 *   out_mean           nullable, n_sounds * n_coeffs f64 (HOST): analyze_mean_mfccs per sound (src/sound.rs:271-286),
 *                      NaN for a sound with no frame (the reference's 0 / 0; ssym_mfcc's own out_mean writes 0 there
 *                      and stays as it is)
 * Limits as ssym_mfcc.  Every failure of the arguments returns SSYM_E_INVALID with a message before device memory is
 * touched, and leaves the host outputs unwritten. */
SSYM_API int32_t ssym_mfcc_batch(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets,
                                 uint32_t n_sounds, double sample_rate, uint32_t n_coeffs, double f_lo, double f_hi,
                                 uint32_t flags, uint64_t *out_frame_offsets, double *out_mfccs, double *out_mean);
/* SoundSequence::new's distances (src/sound.rs:392-398) for a sequence of n_sounds feature blocks:
 * out_dist[i] = cosine_sim_angular(mean_i, mean_{i+1}) (src/sound.rs:59-69), i < n_sounds - 1.  Definitions in
 * csrc/sequence.hip and DESIGN.md section 5.10: mean as analyze_mean_mfccs (NaN for a block without frames), the
 * reference's cosine_sim (squared norms, rulinalg's dot), its clamp (sim < -1 also maps to 1), acos * FRAC_1_PI.
 *   feats, frame_offsets  as ssym_dict_create, f64 (HOST; feats is device memory with SSYM_OUT_DEVICE)
 *   dim                   1 <= dim <= 64
 *   out_mean  nullable, n_sounds * dim (HOST);  out_sim  nullable, n_sounds - 1 (HOST): the clamped similarity before
 *   acos;  out_dist  nullable, n_sounds - 1 (HOST)
 * Every failure of the arguments returns SSYM_E_INVALID with a message before device memory is touched, and leaves
 * the host outputs unwritten. */
SSYM_API int32_t ssym_sequence_distances(ssym_ctx *ctx, const double *feats, const uint64_t *frame_offsets,
                                         uint32_t n_sounds, uint32_t dim, uint32_t flags,
                                         double *out_mean, double *out_sim, double *out_dist);

/* Partitioner: what Partitioner / train_model / discretize_with_model (src/lib.rs:32-151) do --
 * standardise the frames, fit a Gaussian mixture, label every frame with its most likely component (a "letter") and cut
 * the letter string with voting experts.  PARITY UNPINNED: the reference's arithmetic is in un-vendored crates
 * (rusty_machine, voting_experts); the definitions are this library's own, written down in csrc/partition.hip and
 * DESIGN.md section 5.8.  Everything is f64 on the device and deterministic (a second call gives the same bits).
 *   feats        n_frames * dim f64, frame-major (HOST; a device pointer with SSYM_OUT_DEVICE, which then also means the
 *                posteriors / letters / symbols of that call are device memory)
 *   flags        SSYM_OUT_DEVICE; SSYM_GMM_STANDARDIZE: standardise the frames first, with the statistics of the frames
 *                of this call (rusty_machine's Standardizer is fitted on the data it transforms, src/lib.rs:56-60)
 * Limits: 1 <= dim <= 64, 1 <= n_components <= 64, 2 <= alphabet <= 256, depth >= 2, alphabet^depth < 2^63,
 * n < 2^31 symbols.  Every failure returns SSYM_E_INVALID with a message and touches no device memory. */
#define SSYM_GMM_STANDARDIZE 8u
/* Standardizer::default(): per column (x - mean) / sample standard deviation (n - 1); a column whose deviation is 0
 * (or n < 2) maps to 0.  out: n_frames * dim f64 (HOST, or device with SSYM_OUT_DEVICE). */
SSYM_API int32_t ssym_standardize(ssym_ctx *ctx, const double *feats, uint64_t n_frames, uint32_t dim, uint32_t flags,
                         double *out);
/* GaussianMixtureModel with CovOption::Regularized(eps) (the reference: K = 26, eps = 0.1, max_iters 5 in train_model,
 * 1000 in discretize).  init_rows: n_components row indices (HOST) whose frames are the starting means -- the library
 * draws nothing at random.  Needs n_frames >= n_components.  *out is released with ssym_gmm_destroy. */
SSYM_API int32_t ssym_gmm_train(ssym_ctx *ctx, const double *feats, uint64_t n_frames, uint32_t dim,
                       uint32_t n_components, const uint64_t *init_rows, double eps, uint32_t max_iters,
                       uint32_t flags, ssym_gmm **out);
/* the trained parameters (HOST, each nullable): weights [K], means [K][dim], covariances [K][dim][dim], the stored
 * log-likelihood (that of the parameters before the last update; the constant (2 pi)^(dim/2) dropped) and the number
 * of updates made */
SSYM_API int32_t ssym_gmm_get(const ssym_gmm *gmm, double *weights, double *means, double *covs, double *log_lik,
                     uint32_t *iters);
SSYM_API int32_t ssym_gmm_destroy(ssym_ctx *ctx, ssym_gmm *gmm);
/* posteriors (nullable, n_frames * K f64) and letters (n_frames u8: max_index of each posterior row,
 * src/sound.rs:486-495) */
SSYM_API int32_t ssym_gmm_predict(ssym_ctx *ctx, const ssym_gmm *gmm, const double *feats, uint64_t n_frames,
                         uint32_t flags, double *out_post, uint8_t *out_letters);
/* voting experts (cast_votes + split_string) on n symbols < alphabet.  out_votes: nullable, 2 * (n + 1) u32 (HOST):
 * the frequency expert's votes per position 0..n, then the entropy expert's (a position's votes are their sum).
 * out_seg_frames: room for n lengths (HOST); *n_segments of them are written, summing to n (0 segments for n = 0, one
 * for 0 < n < depth). */
SSYM_API int32_t ssym_vote_segments(ssym_ctx *ctx, const uint8_t *symbols, uint64_t n, uint32_t alphabet,
                           uint32_t depth, uint32_t threshold, uint32_t flags, uint32_t *out_votes,
                           uint64_t *out_seg_frames, uint64_t *n_segments);
/* Partitioner::partition_other in frames (multiply by SSYM_MFCC_HOP for samples, src/lib.rs:137): predict + vote in
 * one call, the letters kept on the device; alphabet = the model's n_components.  out_seg_frames: room for n_frames
 * lengths (HOST). */
SSYM_API int32_t ssym_partition(ssym_ctx *ctx, const ssym_gmm *gmm, const double *feats, uint64_t n_frames,
                       uint32_t depth, uint32_t threshold, uint32_t flags, uint64_t *out_seg_frames,
                       uint64_t *n_segments);

/* Sound descriptors: Sound::max_power and Sound::pitch_confidence (src/sound.rs:166-179; the
 * analyses analyze_max_power / analyze_pitch_confidence, :244-269) for a ragged batch of sounds in one call.
 * PARITY UNPINNED for the pitch side: the reference calls vox_box's pitch::<Hanning> (an un-vendored crate); the
 * definition is this library's own, after Boersma (1993), written down in csrc/pitch.hip and DESIGN.md section 5.9.
 * max_power is the reference's arithmetic.  Everything is f64 on the device and deterministic.
 *   samples, sample_offsets  n_sounds + 1 SAMPLE offsets into `samples` (HOST memory, as for ssym_samples_create);
 *                            empty sounds are allowed, n_sounds = 0 is a no-op
 *   rate, f_min, f_max       the lag range [ceil(rate / f_max), floor(rate / f_min)]; the reference passes 44100, 100,
 *                            500 whatever the sound's own rate (src/sound.rs:265)
 *   voicing                  the voicing threshold of the unvoiced candidate (the reference: 0.2)
 *   flags                    SSYM_PITCH_VOICED: a window scores its best voiced strength (0 without one) instead of
 *                            the larger of that and the unvoiced candidate
 * Limits: a finite rate > 0, 0 < f_min < f_max, a finite voicing, 2 <= ceil(rate / f_max) <= floor(rate / f_min) <= 682
 * (three periods per window).  Every failure returns SSYM_E_INVALID with a message and touches no device memory. */
#define SSYM_PITCH_WINDOW 2048
#define SSYM_PITCH_HOP 1024
#define SSYM_PITCH_OCTAVE_COST 0.01
#define SSYM_PITCH_SILENCE 0.03
#define SSYM_POWER_WINDOW 128
#define SSYM_POWER_HOP 64
#define SSYM_PITCH_VOICED 16u
/* full pitch windows of a sound: (n - 2048) / 1024 + 1, 0 below 2048 samples */
SSYM_API int32_t ssym_pitch_num_windows(uint64_t n_samples, uint64_t *out_windows);
/* analyze_max_power + analyze_pitch_confidence (src/sound.rs:244-269) per sound; out_max_power / out_pitch_conf:
 * nullable, n_sounds f64 each (HOST).  A sound shorter than a window has confidence 0, one shorter than 128 samples
 * power 0. */
SSYM_API int32_t ssym_sound_descriptors(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets,
                               uint32_t n_sounds, double rate, double f_min, double f_max, double voicing,
                               uint32_t flags, double *out_max_power, double *out_pitch_conf);
/* the per-window values behind pitch_confidence, sound-major (the windows of sound 0, then of sound 1, ...; counts
 * from ssym_pitch_num_windows), each nullable, f64 (HOST): the best voiced candidate's frequency and strength (both 0
 * when the window has none) and the unvoiced candidate's strength; all three NaN for a window holding a non-finite
 * sample.  flags: as above (the values do not depend on SSYM_PITCH_VOICED). */
SSYM_API int32_t ssym_pitch_track(ssym_ctx *ctx, const double *samples, const uint64_t *sample_offsets,
                         uint32_t n_sounds, double rate, double f_min, double f_max, double voicing, uint32_t flags,
                         double *out_freq, double *out_strength, double *out_unvoiced);

/* Streaming sounds: Sound::push_samples (src/sound.rs:145-164) with the samples, the MFCC
 * frames, the running max_power and the running per-coefficient sums resident on the device.  A stream holds n_lanes
 * independent sounds ("lanes") of one sample_rate / n_coeffs / f_lo / f_hi; the MFCC tables are built and uploaded
 * once, at creation.  A push uploads only the new samples and analyses only the frames and power windows they
 * complete.  After any sequence of pushes a lane holds, bit for bit, what ssym_mfcc (full windows, no
 * SSYM_MFCC_PAD_TAIL), ssym_mfcc_batch (out_mean) and ssym_sound_descriptors (out_max_power) return for the
 * concatenated samples.  The mean is the true mean of the frames held (the reference's running-mean update, :156-158,
 * is not one and is not copied); pitch confidence is not part of a stream.
 * Limits: n_lanes >= 1, a finite sample_rate, otherwise those of ssym_mfcc.  Every failure of the arguments returns
 * SSYM_E_INVALID with a message before device memory is touched; a failed call leaves the stream as it was.  A stream
 * belongs to the context that created it, and every call that takes both wants that context.
 *   capacity_hint_samples  room reserved per lane (0: none); a lane's capacity doubles when it runs out, the old
 *                          samples and frames are copied on the device and never uploaded again */
SSYM_API int32_t ssym_stream_create(ssym_ctx *ctx, uint32_t n_lanes, double sample_rate, uint32_t n_coeffs, double f_lo,
                                    double f_hi, uint64_t capacity_hint_samples, ssym_stream **out);
SSYM_API int32_t ssym_stream_destroy(ssym_ctx *ctx, ssym_stream *st);
/* append samples[sample_offsets[l] .. sample_offsets[l+1]) to lane l, for every lane, and analyse what that completes.
 *   sample_offsets  n_lanes + 1 (HOST), non-decreasing; empty chunks are allowed
 *   flags           SSYM_OUT_DEVICE: out_mfccs is device memory
 *   out_new_frames  nullable, n_lanes u64 (HOST): frames this push added per lane
 *   out_mfccs       nullable: the new frames, lane after lane, sum(out_new_frames) * n_coeffs f64 -- size it with
 *                   ssym_stream_counts and ssym_mfcc_num_frames before the call
 * One synchronisation per call. */
SSYM_API int32_t ssym_stream_push(ssym_ctx *ctx, ssym_stream *st, const double *samples, const uint64_t *sample_offsets,
                                  uint32_t flags, uint64_t *out_new_frames, double *out_mfccs);
/* fill an EMPTY lane with a sound that exists already.  mfccs (nullable, n_frames * n_coeffs f64, HOST): the sound's
 * frames, adopted as given (not analysed again, as :146-148 trusts them); n_frames must not exceed
 * ssym_mfcc_num_frames(n_samples, 0), and frames the samples allow beyond n_frames are analysed by the next push.
 * Without mfccs every frame is analysed now and n_frames is ignored.  Power and sums are computed on the device either
 * way. */
SSYM_API int32_t ssym_stream_seed(ssym_ctx *ctx, ssym_stream *st, uint32_t lane, const double *samples,
                                  uint64_t n_samples, const double *mfccs, uint64_t n_frames);
/* samples and frames held per lane: both nullable, n_lanes u64 each (HOST).  Host arithmetic, no device work. */
SSYM_API int32_t ssym_stream_counts(const ssym_stream *st, uint64_t *out_n_samples, uint64_t *out_n_frames);
/* frames [first_frame, first_frame + n_frames) of a lane: n_frames * n_coeffs f64 (HOST, or device memory with
 * SSYM_OUT_DEVICE) */
SSYM_API int32_t ssym_stream_read(ssym_ctx *ctx, ssym_stream *st, uint32_t lane, uint64_t first_frame, uint64_t n_frames,
                                  uint32_t flags, double *out_mfccs);
/* the resident buffers of a lane (DEVICE pointers, f64; NULL while the lane holds nothing), valid until the next push,
 * seed or destroy of this stream: they feed ssym_partition, ssym_gmm_predict, ssym_sequence_distances (SSYM_OUT_DEVICE)
 * and ssym_queries_create_device / ssym_dict_create_device without a copy */
SSYM_API int32_t ssym_stream_frames_device(const ssym_stream *st, uint32_t lane, const double **out_ptr,
                                           uint64_t *out_n_frames);
SSYM_API int32_t ssym_stream_samples_device(const ssym_stream *st, uint32_t lane, const double **out_ptr,
                                            uint64_t *out_n_samples);
/* out_max_power: nullable, n_lanes f64 (HOST), 0 below 128 samples; out_mean: nullable, n_lanes * n_coeffs f64 (HOST),
 * NaN for a lane without frames, as ssym_mfcc_batch writes it */
SSYM_API int32_t ssym_stream_descriptors(ssym_ctx *ctx, ssym_stream *st, double *out_max_power, double *out_mean);
/* empty one lane; its capacity stays */
SSYM_API int32_t ssym_stream_reset(ssym_ctx *ctx, ssym_stream *st, uint32_t lane);

/* Watching (DESIGN.md section 2 "Watching" and section 5.17): streaming DTW spotting.  A spotter watches n_lanes
 * independent growing sources ("lanes") for every target of one query set.  c, D, st, the squared option and the
 * arithmetic are those of ssym_dtw_spot; i is the absolute frame number within everything the lane has consumed, j a
 * target frame; for lane l and target t the profile is that of "Occurrences": delta(i) = D(i,Fb-1), s(i) = st(i,Fb-1).
 *   resume  : after consuming n frames the spotter holds, per (l,t): n, row n-1 of (D, st) [Fb entries each], the running
 *             best, and the reporting state below.  Consuming frames n ... n+m-1 computes rows n ... n+m-1 from that row.
 *   best    : (cost, start, end) = the first least delta(i) over i ascending from (none, +inf), strict < -- ssym_dtw_spot's
 *             rule: after any push it is ssym_dtw_spot's result for (the frames consumed so far, target), bit for bit
 *   report  : per (l,t), state pend = none, last = none.  For i ascending with (d, s) = (delta(i), s(i)):
 *               1. if pend and s > pend.end:           emit pend;  last = pend.end;  pend = none
 *               2. candidate  iff  d is finite, d <= max_cost[t] (+inf when none is given; NaN fails) and
 *                                  (last = none or s > last)
 *               3. if candidate and (pend = none or d < pend.cost):   pend = (d, s, i)
 *   flush   : if pend: emit pend; last = pend.end; pend = none        (an explicit call: "the lane has ended")
 *   nothing : a target without frames never has a candidate; its best is (+inf, SSYM_NO_MATCH, SSYM_NO_MATCH)
 *             and every row of its profile outputs is (+inf, SSYM_NO_MATCH)
 * So: however the frames of a lane are cut into pushes, the profile, the best after every push and the events (with the
 * push that emits each) are bit for bit those of one push of the whole; the emitted spans of one (l,t) are pairwise
 * disjoint in frames and their ends ascend; every emitted cost has the bits ssym_pair_matrix(exact = 1) gives for (frames
 * start ... end, target); of a run of mutually overlapping candidates the first least is reported; an event is emitted by
 * the push that consumes the first row i with s(i) > pend.end, or by a flush -- never earlier, never lost.  The rule is
 * causal and is NOT ssym_dtw_spot_all's greedy: it decides with what it has seen, and a later, better span that overlaps a
 * span already emitted is rejected by step 2, not preferred.  The cost is NOT normalised by any length.  Features that
 * are not finite as for ssym_dtw_spot, and the stored row carries them across pushes: after a NaN frame a lane reports
 * nothing more for targets of two or more frames until ssym_spotter_reset (a one-frame target loses that row alone),
 * and a NaN target frame makes every end NaN or +inf on every lane: no candidate, no event, no best.
 * ssym_spotter_create: q's resident features are READ BY THE SPOTTER FOR AS LONG AS IT LIVES: destroy the spotter first.
 *   max_cost   HOST memory, n_targets f64, one threshold per target; NULL: none
 *   The state, 12 bytes x (frames of all targets) x n_lanes, is allocated here.  An empty query set is allowed.
 * ssym_spotter_push: appends feats[frame_offsets[l] .. frame_offsets[l+1]) (frames of q's dim, f64, HOST memory whatever
 *   the context's dtype) to lane l, for every lane; empty chunks are allowed.
 *   frame_offsets      n_lanes + 1 (HOST), non-decreasing
 *   out_n_events       the events this call emitted (read them with ssym_spotter_events)
 *   out_profile_cost, out_profile_start   nullable: the new rows' delta (f64) and s (u32), laid out [lane][target][new row]
 *                      (HOST, or device memory with SSYM_OUT_DEVICE)
 * ssym_spotter_follow: for every lane, consumes the frames the stream's lane holds beyond those consumed, read in place
 *   (ssym_stream_frames_device: no copy).  q's dim must equal the stream's n_coeffs and the lane counts must be equal; a
 *   lane that holds fewer frames than were consumed (the stream was reset) is SSYM_E_INVALID: call ssym_spotter_reset.
 *   Outputs as for ssym_spotter_push; the new rows of lane l are the stream's frame count minus ssym_spotter_counts'.
 * ssym_spotter_events: the events of the last push / follow / flush, out_n_events of them, ordered by (lane, target, end);
 *   every output nullable: lane, target, start, end u32, cost f64 (HOST, or device memory with SSYM_OUT_DEVICE).
 * ssym_spotter_flush: the flush of one lane for every target; the lane goes on consuming afterwards.
 * ssym_spotter_best: [n_lanes][n_targets], each output nullable (HOST, or device memory with SSYM_OUT_DEVICE).
 * ssym_spotter_counts: frames consumed per lane, n_lanes u64 (HOST).  Host arithmetic, no device work.
 * ssym_spotter_reset: one lane back to "nothing consumed" (best, pend and last included).
 * Limits: those of ssym_dtw_spot (a dtw context without a band, targets of at most 4096 frames, dim <= 64), and a lane
 * consumes at most 2^31 - 1 = 2147483647 frames (st is u32): beyond them SSYM_E_UNSUPPORTED.  n_lanes = 0, a NaN in
 * max_cost, NULL handles, NULL frame_offsets / out_n_events / feats with frames to read, decreasing offsets, a lane
 * outside the spotter, a handle of another context: SSYM_E_INVALID -- all with a message, before device memory is touched
 * and with the spotter as it was.  The profile of a call lives in device scratch at 12 bytes per (pair, new row); a push
 * whose profile would exceed 512 MiB runs as several slices of rows in the same call, with the same results.  Two
 * synchronisations per slice (the events are counted, the log grown, then written).  ssym_get_timings afterwards:
 * main_ms = the forward kernel(s), reduce_ms = the reporting, n_pairs = n_lanes * n_targets. */
SSYM_API int32_t ssym_spotter_create(ssym_ctx *ctx, const ssym_queries *q, uint32_t n_lanes, const double *max_cost,
                                     ssym_spotter **out);
SSYM_API int32_t ssym_spotter_destroy(ssym_ctx *ctx, ssym_spotter *sp);
SSYM_API int32_t ssym_spotter_push(ssym_ctx *ctx, ssym_spotter *sp, const double *feats, const uint64_t *frame_offsets,
                                   uint32_t flags, uint64_t *out_n_events, double *out_profile_cost,
                                   uint32_t *out_profile_start);
SSYM_API int32_t ssym_spotter_follow(ssym_ctx *ctx, ssym_spotter *sp, const ssym_stream *stream, uint32_t flags,
                                     uint64_t *out_n_events, double *out_profile_cost, uint32_t *out_profile_start);
SSYM_API int32_t ssym_spotter_events(ssym_ctx *ctx, const ssym_spotter *sp, uint32_t *out_lane, uint32_t *out_target,
                                     double *out_cost, uint32_t *out_start, uint32_t *out_end, uint32_t flags);
SSYM_API int32_t ssym_spotter_flush(ssym_ctx *ctx, ssym_spotter *sp, uint32_t lane, uint64_t *out_n_events);
SSYM_API int32_t ssym_spotter_best(ssym_ctx *ctx, const ssym_spotter *sp, double *out_cost, uint32_t *out_start,
                                   uint32_t *out_end, uint32_t flags);
SSYM_API int32_t ssym_spotter_counts(const ssym_spotter *sp, uint64_t *out_frames);
SSYM_API int32_t ssym_spotter_reset(ssym_ctx *ctx, ssym_spotter *sp, uint32_t lane);

/* Paced watching (DESIGN.md section 2 "Paced watching" and section 5.20): ssym_spotter_create with a step pattern.
 * SSYM_STEP_SYMMETRIC is ssym_spotter_create itself: one host path, the same kernels, the same bits.  With SSYM_STEP_PACED
 * the spotter watches under the pattern of "Paced spotting": c, the squared option, the arithmetic and the states N, H,
 * E, P are those, word for word; i is the absolute frame number within everything the lane has consumed;
 * delta(i) = E(i,Fb-1).value and s(i) = E(i,Fb-1).start.
 *   resume  : after consuming n frames the spotter holds, per (l,t): n, rows n-1 and n-2 of E (value f64, start u32; Fb
 *             entries each; a row that does not exist yet is (+inf, none)), the running best, pend, last.  Consuming
 *             frames n ... n+m-1 computes rows n ... n+m-1 from those two rows.
 *   best    : the first least delta(i), i ascending from (none, +inf), strict < -- after any push it is
 *             ssym_dtw_spot_step(SSYM_STEP_PACED)'s result for (the frames consumed so far, target), bit for bit
 *   report, flush, nothing : those of "Watching" above, unchanged, on this (delta, s)
 * So: however a lane is cut into pushes, the profile, the best after every push and the events (with the push that emits
 * each) are bit for bit those of one push; every emitted span has between floor((Fb-1)/2) + 1 and 2 Fb - 1 frames, the
 * spans of one (l,t) are pairwise disjoint and their ends ascend; every emitted cost has the bits
 * ssym_dtw_align_step(SSYM_STEP_PACED) gives for (frames start ... end, target), so a span goes straight into that call.
 * Every path has Fb cells: a caller that wants one per-frame threshold x for targets of every length passes
 * max_cost[t] = x * Fb[t] (max_cost stays a sum here, as costs do) and +inf for a target without frames.
 * Features that are not finite as for "Paced spotting", carried across pushes by the two stored rows: the recurrence has
 * no edge from row i to row i in the next column but through N, so a NaN or infinite source frame poisons a bounded
 * stretch of rows only, after which the lane spots again WITHOUT ssym_spotter_reset; a poisoned target frame is on every
 * path, so that target never has a candidate on any lane.  No read leaves its buffer.
 * The spotter remembers its step: push, follow, events, flush, best, counts, reset and destroy act by it.
 * An unknown step: SSYM_E_INVALID.  Limits with SSYM_STEP_PACED: targets of at most 2048 frames (two hand-off rows
 * take 24 bytes of LDS per target frame): a longer one is SSYM_E_UNSUPPORTED at creation, before any device work.
 * Every other limit, refusal and output is that of "Watching".  The state is
 * 24 bytes x (frames of all targets) x n_lanes under SSYM_STEP_PACED and stays 12 under SSYM_STEP_SYMMETRIC. */
SSYM_API int32_t ssym_spotter_create_step(ssym_ctx *ctx, const ssym_queries *q, uint32_t n_lanes, const double *max_cost,
                                          uint32_t step, ssym_spotter **out);

/* Live cover (DESIGN.md section 2 "Live cover" and section 5.24): the cover of targets that grow.  A coverer holds n_lanes
 * growing targets against ONE resident dictionary and reports every piece with the push after which no longer recording
 * could change it.  c, w, M, src, best, the tie rules and the arithmetic are those of "Cover" above, word for word.  For one
 * lane, X is everything consumed so far, n its frame count, W = 2 max(Fmax, 1), Fmax the dictionary's longest segment at
 * creation:
 *   resume   : the lane holds n, its last W-1 frames, best(e) for the last W ends, the back-pointers (L, src, M) of every
 *              frame after the committed end, done (the last committed end, -1 at first) and lastFinite (the largest e with
 *              a finite best(e), -1 at first: best(-1) = 0).  Consuming frames n ... n+m-1 computes M(s,L) for every window
 *              that ends in them and best(e) and the back-pointers for e = n ... n+m-1, exactly as "Cover" does.
 *   horizon  : H(n) = { e : max(-1, n-W) <= e <= n-1, best(e) finite }   (-1 belongs to it while n < W)
 *   walk(e)  : the pieces the back-pointers give from e down to -1, in ascending start   (walk(-1) is empty)
 *   commit   : C(n) = the longest common prefix of walk(e) over e in H(n); H(n) empty: nothing new.  A push emits the pieces
 *              of C(n) not emitted before, and done = the end of the last of them.
 *   flush    : emits the pieces of walk(lastFinite) not emitted before.  The lane has then ENDED: it consumes nothing more
 *              until ssym_coverer_reset (ssym_coverer_push with frames for it: SSYM_E_INVALID; ssym_coverer_follow skips it).
 *   best     : total = best(n-1) (+inf for n = 0 or when not finite), covered = lastFinite + 1, committed = done + 1
 * So: (1) after any push, total has the bits ssym_dtw_cover returns for the frames consumed so far as one target; (2) C(n)
 * depends on the frames consumed, not on how they were cut into pushes, slices or lanes, and only grows; (3) never revised:
 * the cover of every longer recording that has one starts with C(n), pieces, cuts and cost bits; (4) with best(n-1) finite
 * the pieces emitted from reset to flush are ssym_dtw_cover's for the whole, else they are its cover of X[0 ... lastFinite];
 * (5) a piece's cost is the paced alignment's for the cut; (6) a NaN or +-inf target frame ends the lane's coverable prefix
 * before it: nothing is committed past it, total stays +inf, the flush gives the cover of the prefix, other lanes are
 * untouched; a dictionary segment with a NaN frame is never chosen; no read leaves its buffer; (7) device state per lane is
 * the W-1 tail frames, the ring of best values and the back-pointers of the uncommitted stretch n-1-done, held in a ring of
 * frames whose capacity is a power of two, 1024 at least, grown (doubling) when the uncommitted stretch plus a slice's
 * frames would not fit; nothing scales with the stream.  The uncommitted stretch has no hard bound.
 *
 * ssym_coverer_create: dict's resident features are READ BY THE COVERER FOR AS LONG AS IT LIVES: destroy the coverer first.
 *   A dictionary appended to since: SSYM_E_INVALID at the next push / follow.  piece_penalty as for ssym_dtw_cover.
 * ssym_coverer_push: appends feats[frame_offsets[l] .. frame_offsets[l+1]) (frames of the dictionary's dim, f64, HOST
 *   memory whatever the context's dtype) to lane l, for every lane; an empty range leaves a lane alone.
 *   out_n_pieces   the pieces this call emitted (read them with ssym_coverer_pieces)
 * ssym_coverer_follow: for every lane, consumes the frames the stream's lane holds beyond those consumed, device to device.
 *   The stream must belong to ctx and have the coverer's lanes and n_coeffs = the dictionary's dim; a lane that holds
 *   fewer frames than were consumed (the stream was reset) is SSYM_E_INVALID: call ssym_coverer_reset.
 * ssym_coverer_pieces: the pieces of the last push / follow / flush, out_n_pieces of them, ordered by (lane, start); each
 *   output nullable (HOST, or device memory with SSYM_OUT_DEVICE).  start / end count frames of the lane since its reset.
 * ssym_coverer_flush: the flush of one lane.
 * ssym_coverer_best: [n_lanes] each, nullable (HOST, or device memory with SSYM_OUT_DEVICE).
 * ssym_coverer_counts: frames consumed per lane (n_lanes u64) and the capacity of the back-pointer ring in frames (one
 *   u64), HOST, each nullable.  Host arithmetic, no device work.
 * ssym_coverer_reset: one lane back to "nothing consumed".
 * Limits, checked at creation before any device work: a dtw context without a band, dim <= 64, every dictionary segment of
 * at most 128 frames (kCoverMaxSourceFrames), at most 65535 lanes, and lanes x 2 Fmax x 2 Fmax x 12 bytes <= 512 MiB:
 * SSYM_E_UNSUPPORTED beyond them and on a refcos context.  An empty dictionary: SSYM_E_EMPTY_DICT.  A NaN, negative or
 * infinite piece_penalty: SSYM_E_INVALID.  A lane consumes at most 2^31 - 1 frames (SSYM_E_UNSUPPORTED beyond).  NULL
 * handles, decreasing offsets, a lane outside the coverer, a handle of another context, a stream whose lanes or n_coeffs
 * differ: SSYM_E_INVALID with a message, the coverer as it was and the outputs unwritten.
 * The tables of one call are lanes x (W - 1 + new frames) x W x 12 bytes per source block; a push that would pass the
 * cover's 512 MiB runs as several slices of frames in the same call, with a commit after each and the same results.  What
 * earlier slices consumed stays consumed and is in the log (after any failure of a later slice out_n_pieces counts what the
 * earlier ones logged).  One synchronisation per slice.  ssym_get_timings afterwards: main_ms = the forward pass (gather
 * and fold included), reduce_ms = chain, commit and emission, n_pairs = n_sources x the frames the call consumed.
 *
 * ssym_coverer_create_gaps: a coverer whose chain takes the gap candidate of "Cover with gaps" at gap_cost per frame (>= 0 and
 *   finite, or +inf, which is ssym_coverer_create; NaN, negative or -inf: SSYM_E_INVALID).  Every other ssym_coverer_* call
 *   works on it unchanged; "ssym_dtw_cover" above then reads "ssym_dtw_cover_gaps with the same gap_cost".  A gap frame is a
 *   piece of one frame and 1 <= W, so the horizon argument holds as it stands and (1) to (5) and (7) hold with gaps;
 *   ssym_coverer_pieces reports a gap frame as (lane, SSYM_COVER_GAP, e, e, gap_cost).  With a finite gap_cost every best(e)
 *   is finite, so lastFinite = n - 1 and covered = n, and (6) is replaced by: a NaN or +-inf frame becomes a gap frame and
 *   the lane goes on; other lanes are untouched. */
SSYM_API int32_t ssym_coverer_create(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty,
                                     ssym_coverer **out);
SSYM_API int32_t ssym_coverer_create_gaps(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty,
                                          double gap_cost, ssym_coverer **out);
SSYM_API int32_t ssym_coverer_destroy(ssym_ctx *ctx, ssym_coverer *cv);
SSYM_API int32_t ssym_coverer_push(ssym_ctx *ctx, ssym_coverer *cv, const double *feats, const uint64_t *frame_offsets,
                                   uint32_t flags, uint64_t *out_n_pieces);
SSYM_API int32_t ssym_coverer_follow(ssym_ctx *ctx, ssym_coverer *cv, const ssym_stream *stream, uint32_t flags,
                                     uint64_t *out_n_pieces);
SSYM_API int32_t ssym_coverer_pieces(ssym_ctx *ctx, const ssym_coverer *cv, uint32_t *out_lane, uint32_t *out_src,
                                     uint32_t *out_start, uint32_t *out_end, double *out_cost, uint32_t flags);
SSYM_API int32_t ssym_coverer_flush(ssym_ctx *ctx, ssym_coverer *cv, uint32_t lane, uint64_t *out_n_pieces);
SSYM_API int32_t ssym_coverer_best(ssym_ctx *ctx, const ssym_coverer *cv, double *out_total, uint32_t *out_covered,
                                   uint32_t *out_committed, uint32_t flags);
SSYM_API int32_t ssym_coverer_counts(const ssym_coverer *cv, uint64_t *out_frames, uint64_t *out_capacity);
SSYM_API int32_t ssym_coverer_reset(ssym_ctx *ctx, ssym_coverer *cv, uint32_t lane);

/* Live mosaic (DESIGN.md section 2 "Live mosaic" and section 5.26): the mosaic of targets that grow.  A mosaicker holds
 * n_lanes growing targets against ONE resident dictionary and reports every target frame with the push after which no longer
 * recording could change it.  c, S, P, open, Q, H, N, E, best, arg, the tie rules and the arithmetic are those of "Mosaic"
 * above, word for word.  For one lane, X is everything consumed so far and n its frame count:
 *   resume   : the lane holds n, E(., n-1) and N(., n-1), best(n-1), the direction byte of every (g, j) and arg(j) for every
 *              column j after the committed column, done (the last committed column, -1 at first), the committed tip (the
 *              key at done; walks stop at column done + 1, so it need not be stored) and lastFinite (the largest j with a
 *              finite best(j), -1 at first).  Consuming frames n ... n+m-1 runs columns n ... n+m-1 exactly as "Mosaic"
 *              does.
 *   key      : a position of the backward walk at column j: (g, H), (g, N) or GAP.  A walk steps from a key at column j to
 *              one at column j-1 by the "backward" rule of "Mosaic".  Two walks that share a key at a column are the same
 *              from there back.
 *   live(n)  : S' = piece_penalty + best(n-1), as the next column will form it.  Every g with E(g, n-1) finite and <= S'
 *              gives a hypothesis in the state byte bit 0 says (H if H < N, else N); every g whose bit 0 is set and whose
 *              N(g, n-1) is finite and <= S' gives one in state N; GAP at column n-1 is one if arg(n-1) = GAP and best(n-1)
 *              is finite.  NaN is never live.
 *   commit   : c(n) = the largest column <= n-1 at which all walks of live(n) hold the same key, -1 if there is none; live(n)
 *              empty: unchanged.  A push emits frames done+1 ... c(n), each with the outputs ssym_dtw_mosaic gives it: src
 *              (or SSYM_COVER_GAP), frame, cost, and whether a piece or gap frame starts there.  Then done = c(n).
 *   dead     : best(n-1) not finite makes every later column +inf (E and N are all non-finite and S = +inf); it cannot
 *              happen with a finite gap_cost.  A dead lane goes on counting frames but stores nothing more and commits
 *              nothing more.
 *   flush    : emits the rest of the walk from arg(lastFinite) at column lastFinite.  The lane has then ENDED until
 *              ssym_mosaicker_reset (ssym_mosaicker_push with frames for it: SSYM_E_INVALID; ssym_mosaicker_follow skips it).
 *   best     : total = best(n-1) (+inf for n = 0 or when not finite), covered = lastFinite + 1, committed = done + 1
 * Why: a state above S' is never used by column n.  E: as the P of a successor it is > S' and that successor opens, else the
 * other predecessor was taken.  N: H(g,n) = c + N(g,n-1) wins only if it is < c + Q with Q <= S', and rounding is monotone.
 * So every mosaic of every longer X passes through a live state at column n-1, and hence through the common key at c(n).
 * So: (1) after any push, total has the bits ssym_dtw_mosaic returns for the frames consumed so far as one target; (2) c(n)
 * depends on the frames consumed, not on how they were cut into pushes, slices or lanes, and only grows; (3) frames once
 * emitted are never revised; (4) from reset to flush the frames emitted are ssym_dtw_mosaic's six arrays for the whole
 * target, and if the lane died those for X[0 ... lastFinite]; (5) device state per lane is 32 G bytes of E / N, 24 G + 24 of
 * the commit's key lists, and a ring of G + 4 + 8 dim bytes per uncommitted column (direction bytes, arg and the target
 * frame, which the emitted frame cost is formed from): nothing grows with the stream.  The uncommitted stretch has no hard
 * bound but the memory below.
 *
 * ssym_mosaicker_create: dict's resident features are READ BY THE MOSAICKER FOR AS LONG AS IT LIVES: destroy the mosaicker
 *   first.  The transposed source frames and pos are made here, once.  A dictionary appended to since: SSYM_E_INVALID at
 *   the next push / follow.  piece_penalty and gap_cost as for ssym_dtw_mosaic; a gap_cost of +inf means no gaps.
 * ssym_mosaicker_push: appends feats[frame_offsets[l] .. frame_offsets[l+1]) (frames of the dictionary's dim, f64, HOST
 *   memory whatever the context's dtype) to lane l, for every lane; an empty range leaves a lane alone.
 *   out_n_frames   the frames this call emitted (read them with ssym_mosaicker_frames)
 * ssym_mosaicker_follow: for every lane, consumes the frames the stream's lane holds beyond those consumed, device to
 *   device; the stream as for ssym_coverer_follow.
 * ssym_mosaicker_frames: the frames of the last push / follow / flush, out_n_frames of them, ordered by (lane, column); each
 *   output nullable (HOST, or device memory with SSYM_OUT_DEVICE).  column counts the lane's frames since its reset;
 *   (src, frame, cost) are ssym_dtw_mosaic's out_src, out_frame and out_frame_cost of that target frame; start is 1 where a
 *   piece or a gap frame starts, else 0.
 * ssym_mosaicker_flush: the flush of one lane; ssym_coverer_flush's rules.
 * ssym_mosaicker_best: [n_lanes] each, nullable (HOST, or device memory with SSYM_OUT_DEVICE).
 * ssym_mosaicker_counts: frames consumed per lane (n_lanes u64) and the capacity of the ring in columns (one u64), HOST,
 *   each nullable.  Host arithmetic, no device work.
 * ssym_mosaicker_reset: one lane back to "nothing consumed".
 * Limits, checked at creation before any device work: a dtw context without a band, dim <= 64, at most 65535 lanes, and the
 * state with a ring of 16 columns within 512 MiB: SSYM_E_UNSUPPORTED beyond them.  An empty dictionary: SSYM_E_EMPTY_DICT.
 * Prices as for ssym_dtw_mosaic.  A lane consumes at most 2^31 - 1 frames.  Refusals and their order are the coverer's.
 * The ring starts at the largest power of two <= 1024 columns with lanes x columns x (G + 4) <= 64 MiB (16 at least) and
 * doubles when the uncommitted stretch plus a slice would not fit.  Everything the mosaicker owns beside a call's frame log
 * stays within 512 MiB, the ring it leaves beside the new one while it doubles included: a call runs in slices with a
 * commit after each, a slice is shortened to fit, and if the uncommitted stretch alone fills the cap the call returns
 * SSYM_E_UNSUPPORTED with a message that says to flush -- what earlier slices consumed stays consumed and is in the log
 * (after any failure of a later slice out_n_frames counts what the earlier ones logged).  One synchronisation per slice.  ssym_get_timings afterwards: main_ms = the
 * forward pass, reduce_ms = commit and emission, n_pairs = G x the frames the call consumed. */
SSYM_API int32_t ssym_mosaicker_create(ssym_ctx *ctx, const ssym_dict *dict, uint32_t n_lanes, double piece_penalty,
                                       double gap_cost, ssym_mosaicker **out);
SSYM_API int32_t ssym_mosaicker_destroy(ssym_ctx *ctx, ssym_mosaicker *mk);
SSYM_API int32_t ssym_mosaicker_push(ssym_ctx *ctx, ssym_mosaicker *mk, const double *feats, const uint64_t *frame_offsets,
                                     uint32_t flags, uint64_t *out_n_frames);
SSYM_API int32_t ssym_mosaicker_follow(ssym_ctx *ctx, ssym_mosaicker *mk, const ssym_stream *stream, uint32_t flags,
                                       uint64_t *out_n_frames);
SSYM_API int32_t ssym_mosaicker_frames(ssym_ctx *ctx, const ssym_mosaicker *mk, uint32_t *out_lane, uint32_t *out_column,
                                       uint32_t *out_src, uint32_t *out_frame, double *out_cost, uint32_t *out_start,
                                       uint32_t flags);
SSYM_API int32_t ssym_mosaicker_flush(ssym_ctx *ctx, ssym_mosaicker *mk, uint32_t lane, uint64_t *out_n_frames);
SSYM_API int32_t ssym_mosaicker_best(ssym_ctx *ctx, const ssym_mosaicker *mk, double *out_total, uint32_t *out_covered,
                                     uint32_t *out_committed, uint32_t flags);
SSYM_API int32_t ssym_mosaicker_counts(const ssym_mosaicker *mk, uint64_t *out_frames, uint64_t *out_capacity);
SSYM_API int32_t ssym_mosaicker_reset(ssym_ctx *ctx, ssym_mosaicker *mk, uint32_t lane);

/* Live resynthesis (DESIGN.md section 2 "Live resynthesis" and section 5.27): committed mosaic frames to audio, push by push.
 * A resynthesiser holds n_lanes lanes against ONE resident sample store.  A lane receives committed frames in column order --
 * from a mosaicker's frame log device to device (ssym_resynth_take) or from host arrays (ssym_resynth_push) -- and releases
 * output samples as soon as their bits can no longer change.  From reset to flush a lane's output is, bit for bit, what the
 * window calls below "Sample windows" give piece by piece for the finished mosaic.  HOP = 256, BIN = 1024 and w[] are those
 * of "Warped reconstruction", and so are its taps / value / pcm rules; the pos[] chain is that of "WSOLA reconstruction";
 * the window rule is that of "Sample windows" -- all word for word.
 *   input    : each frame is (src, frame, start), the mosaicker's log words.  src = SSYM_COVER_GAP is a gap frame.  A tile
 *              starts at every frame with start = 1.  A sounding tile a...b has map[j] = frame_j, first = map[a], last =
 *              map[b]; within a tile map steps by 0, 1 or 2, never by 0 twice in a row.
 *   output   : of a lane that ended with N samples: tile i owns (b - a + 1) * HOP samples, the last tile N - a * HOP.  A
 *              sounding tile is the _spans call's output with the window [min(first * HOP, n_src), min((last + 1) * HOP,
 *              n_src)) of sound src, the map map - first, and pos[0] = 0 at the tile's first frame.  A gap tile is +0.0.  A
 *              lane without frames is N zeros.  Hop j of the lane is samples [j * HOP, (j + 1) * HOP); its taps are frames
 *              max(a, j - 3) ... j of its own tile only.
 *   release  : L is the map value of the latest frame pushed into the open tile.  Hop j is released, in column order, when
 *              its tile is closed (a later frame with start = 1 has arrived in the lane, or the lane is flushed), or when
 *              map[j] + R <= L with R = 2 for search = 0 and R = floor((search + 1279) / 256) otherwise (5 up to 256, 6 up to
 *              512), or at once when it is a gap frame.  An open tile is rendered with the window end (L + 1) * HOP, clipped
 *              to n_src.
 *   why      : search = 0: a tap j' of hop j reads source hops up to map[j'] + (j - j'); any two consecutive steps sum to at
 *              least 1, so that is at most map[j] + 2.  search > 0: the template reads up to pos[j-1] + HOP + BIN - 1, at
 *              most map[j] * HOP + search + 1279; candidates, admissibility and taps reach less far.  Every read that decides
 *              a released hop therefore lies below (L + 1) * HOP: a later `last` cannot change it.
 *   so       : at most 2 R hops of a lane are held back (4 for the plain warp, 12 for WSOLA), R on a diagonal map; what is
 *              released depends on the frames consumed, not on how they were cut into pushes; device state is a ring of 16
 *              frames per lane (the unreleased frames and the three before them with their pos).
 *   flush    : (lane, total_samples) closes the open tile and releases the rest, the tail total_samples - frames * HOP
 *              included.  The lane has then ENDED until ssym_resynth_reset.
 *
 * ssym_resynth_create: any context (as ssym_reconstruct_warped).  store is READ BY THE RESYNTHESISER FOR AS LONG AS IT LIVES:
 *   destroy the resynthesiser first.  search: ssym_reconstruct_wsola's S, at most 512 (beyond: SSYM_E_INVALID); 0 is the plain
 *   warp.  n_lanes 1 ... 65535 (0: SSYM_E_INVALID; more: SSYM_E_UNSUPPORTED).  An empty store: SSYM_E_EMPTY_DICT.  Refusals
 *   come before any device work.
 * ssym_resynth_push: n_frames frames in HOST arrays ordered by (lane, column).  Refusals, all SSYM_E_INVALID, nothing
 *   consumed, the earliest entry's first fault reported, per entry in this order: a lane outside the lanes or out of order;
 *   column does not continue the lane's count; the lane has ended; the lane's first frame has start = 0; src is neither a
 *   sound of the store nor SSYM_COVER_GAP; a frame with start = 0 that names another sound than its tile, follows a gap
 *   frame, or breaks the 0 / 1 / 2 rule.  A lane consumes at most 2^31 - 1 frames (SSYM_E_UNSUPPORTED).
 *   out_n_samples  the samples this call released (read them with ssym_resynth_samples)
 * ssym_resynth_take: consumes the mosaicker's last frame log (that of its last push / follow / flush) where it lies, in
 *   device memory: no frame goes through the host.  The mosaicker must be of the same context and have as many lanes, and
 *   every lane's log must continue the columns the lane has consumed: SSYM_E_INVALID otherwise.  Taking the same log twice:
 *   SSYM_E_INVALID.  The frames of a mosaicker obey the tile rules by construction and are not checked again.
 * ssym_resynth_samples: the samples of the last push / take / flush, lane by lane: lane l's are
 *   [out_lane_offsets[l], out_lane_offsets[l+1]) of out_samples (f64) and out_pcm32 (warp_pcm32 of each).  out_lane_offsets
 *   ([n_lanes + 1], always HOST), out_samples and out_pcm32 (HOST, or device memory with SSYM_OUT_DEVICE) are each nullable.
 * ssym_resynth_flush: the flush of one lane.  total_samples < frames * HOP, a lane outside the lanes, a lane that has ended
 *   or out_n_samples NULL: SSYM_E_INVALID.
 * ssym_resynth_counts: frames consumed and samples released per lane since its reset (n_lanes u64 each, HOST, nullable).
 *   Host arithmetic, no device work.
 * ssym_resynth_reset: one lane back to "nothing consumed".
 * One synchronisation per call: the released counts depend on device data and come back with it.  ssym_get_timings
 * afterwards: main_ms = the search, reduce_ms = staging and synthesis, n_pairs = the frames the call consumed.  A call's hop
 * list (32 bytes per released hop) and its samples (12 bytes each) are scratch of the object, reused by the next call. */
SSYM_API int32_t ssym_resynth_create(ssym_ctx *ctx, const ssym_samples *store, uint32_t n_lanes, uint32_t search,
                                     ssym_resynth **out);
SSYM_API int32_t ssym_resynth_destroy(ssym_ctx *ctx, ssym_resynth *rs);
SSYM_API int32_t ssym_resynth_push(ssym_ctx *ctx, ssym_resynth *rs, const uint32_t *lane, const uint32_t *column,
                                   const uint32_t *src, const uint32_t *frame, const uint32_t *start, uint64_t n_frames,
                                   uint64_t *out_n_samples);
SSYM_API int32_t ssym_resynth_take(ssym_ctx *ctx, ssym_resynth *rs, const ssym_mosaicker *mk, uint64_t *out_n_samples);
SSYM_API int32_t ssym_resynth_samples(ssym_ctx *ctx, const ssym_resynth *rs, uint64_t *out_lane_offsets, double *out_samples,
                                      int32_t *out_pcm32, uint32_t flags);
SSYM_API int32_t ssym_resynth_flush(ssym_ctx *ctx, ssym_resynth *rs, uint32_t lane, uint64_t total_samples,
                                    uint64_t *out_n_samples);
SSYM_API int32_t ssym_resynth_counts(const ssym_resynth *rs, uint64_t *out_frames, uint64_t *out_samples);
SSYM_API int32_t ssym_resynth_reset(ssym_ctx *ctx, ssym_resynth *rs, uint32_t lane);

/* Live envelope following (DESIGN.md section 2 "Live envelope following" and section 5.29): ssym_follow_envelope's resumable
 * form.  A follower holds n_lanes lanes and one max_gain.  A lane receives two growing signals: y, the resynthesis, and x, the
 * reference (the target's own samples).  Either arrives in any amounts: not hop-aligned, neither has to lead the other.  ny
 * and nx are the counts consumed since the lane's reset.  HOP, BIN, w[] and the energy, gain, sample and pcm rules are those
 * of "Envelope following" above, word for word.
 *   settle   : with h = floor(min(ny, nx) / HOP), before a flush: boundary b is settled when (b + 2)*HOP <= min(ny, nx) --
 *              max(0, h - 1) boundaries so far -- and hop j is released when boundaries j and j + 1 are settled -- max(0, h - 2)
 *              hops so far.  The counts are host arithmetic on how much was consumed, never on sample values or on how the
 *              samples were cut into pushes.
 *   flush    : ends the lane with n = ny.  Every remaining boundary b <= J = ceil(n / HOP) is computed with the offline
 *              clipping: k >= n is left out, x[k] reads +0.0 for k >= nx, x at or beyond n is dropped unread.  The rest of y
 *              leaves, the tail included.  A lane flushed at ny = 0 releases nothing.  The lane has then ENDED until
 *              ssym_follower_reset.
 *   why      : a settled boundary's window [(b-2)*HOP, (b+2)*HOP) lies wholly below both counts: no later sample and no later
 *              n enters its sum; terms with k < 0 are +0.0 in both routes.  So from reset to flush a lane's samples and gains
 *              are ssym_follow_envelope's for (y[0..ny), x[0..nx)), bit for bit.  Releasing one hop earlier changes bits.
 *   state    : per lane and signal the samples from (r - 2)*HOP on (r: the hops released; g(r) sits in the lane's record), in
 *              a ring indexed by absolute sample index modulo a power-of-two capacity shared by the lanes: at least 2048, grown
 *              to the longest held stretch plus the call's samples.  Both rings of an object stay within 512 MiB, so at most
 *              16384 lanes are accepted, and a call that would pass the cap is refused with nothing consumed.  A lane consumes
 *              fewer than 2^40 samples per signal.
 *
 * ssym_follower_create: any context.  max_gain finite and at least 1, n_lanes 1 ... 16384 (0: SSYM_E_INVALID; more:
 *   SSYM_E_UNSUPPORTED).  Refusals come before any device work, in the order ctx, out, max_gain, lanes.
 * ssym_follower_push: lane l consumes samples[sample_offsets[l] ... sample_offsets[l+1]) of y and ref[ref_offsets[l] ...
 *   ref_offsets[l+1]) of x.  Both offset arrays are [n_lanes + 1] u64 (HOST), start at 0 and do not decrease.  samples and ref
 *   are HOST memory, or device memory with SSYM_FOLLOW_SAMPLES_DEVICE / SSYM_FOLLOW_REF_DEVICE; either may be NULL when it
 *   holds nothing.  Refusals are SSYM_E_INVALID or SSYM_E_UNSUPPORTED, nothing is consumed, the earliest fault is reported, in
 *   this order: the handle, unknown flag bits, NULL offsets or count, the offsets' start, then lane by lane (a decrease; the
 *   lane has ended; the 2^40 limit, SSYM_E_UNSUPPORTED), the ring cap (SSYM_E_UNSUPPORTED), NULL arrays.
 *   out_n_samples  the samples this call released over all lanes (read them with ssym_follower_samples)
 * ssym_follower_flush: the flush of one lane.  A lane outside the lanes, a lane that has ended or out_n_samples NULL:
 *   SSYM_E_INVALID.
 * ssym_follower_samples: what the last push or flush released, lane by lane: lane l's samples are [out_lane_offsets[l],
 *   out_lane_offsets[l+1]) of out_samples (f64) and out_pcm32 (ssym_reconstruct's conversion of each); the gains of the
 *   boundaries that call settled are [out_gain_offsets[l], out_gain_offsets[l+1]) of out_gain, in boundary order.  Every
 *   pointer is nullable.  The two offset arrays ([n_lanes + 1] u64) are always HOST; the rest is HOST memory, or device
 *   memory with SSYM_OUT_DEVICE.
 * ssym_follower_counts: ny, nx and the samples released per lane since its reset (n_lanes u64 each, HOST, nullable).  Host
 *   arithmetic, no device work.
 * ssym_follower_reset: one lane back to "nothing consumed".
 * One synchronisation per push or flush (a call whose sample log has to grow waits once more, as the resynthesiser's).
 * ssym_get_timings afterwards: main_ms = the gain kernel, reduce_ms = append plus
 * apply, n_pairs = the boundaries the call settled.  A call's samples (12 bytes each) and gains are scratch of the object,
 * reused by the next call. */
SSYM_API int32_t ssym_follower_create(ssym_ctx *ctx, uint32_t n_lanes, double max_gain, ssym_follower **out);
SSYM_API int32_t ssym_follower_destroy(ssym_ctx *ctx, ssym_follower *fl);
SSYM_API int32_t ssym_follower_push(ssym_ctx *ctx, ssym_follower *fl, const double *samples, const uint64_t *sample_offsets,
                                    const double *ref, const uint64_t *ref_offsets, uint32_t flags, uint64_t *out_n_samples);
SSYM_API int32_t ssym_follower_flush(ssym_ctx *ctx, ssym_follower *fl, uint32_t lane, uint64_t *out_n_samples);
SSYM_API int32_t ssym_follower_samples(ssym_ctx *ctx, const ssym_follower *fl, uint64_t *out_lane_offsets, double *out_samples,
                                       int32_t *out_pcm32, uint64_t *out_gain_offsets, double *out_gain, uint32_t flags);
SSYM_API int32_t ssym_follower_counts(const ssym_follower *fl, uint64_t *out_ny, uint64_t *out_nx, uint64_t *out_released);
SSYM_API int32_t ssym_follower_reset(ssym_ctx *ctx, ssym_follower *fl, uint32_t lane);

#ifdef __cplusplus
}
#endif
#endif /* SOUNDSYM_AMD_H */
