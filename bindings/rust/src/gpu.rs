//! `extern "C"` declarations, 1:1 with `include/soundsym_amd.h` (ABI version 2).
//!
//! What each call replaces in the crate (`src/sound.rs`): see the header's comments and `INTEGRATION.md`
//! section 3.  Nothing here allocates or frees Rust memory on the other side of the boundary; the library
//! copies caller buffers at create time and never unwinds into the caller.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_void};

#[repr(C)] pub struct SsymCtx { _p: [u8; 0] }
#[repr(C)] pub struct SsymDict { _p: [u8; 0] }
#[repr(C)] pub struct SsymQueries { _p: [u8; 0] }
#[repr(C)] pub struct SsymSamples { _p: [u8; 0] }
#[repr(C)] pub struct SsymComm { _p: [u8; 0] }
#[repr(C)] pub struct SsymLocalGroup { _p: [u8; 0] }
#[repr(C)] pub struct SsymGmm { _p: [u8; 0] }
#[repr(C)] pub struct SsymStream { _p: [u8; 0] }
#[repr(C)] pub struct SsymSpotter { _p: [u8; 0] }
#[repr(C)] pub struct SsymCoverer { _p: [u8; 0] }
#[repr(C)] pub struct SsymMosaicker { _p: [u8; 0] }
#[repr(C)] pub struct SsymResynth { _p: [u8; 0] }
#[repr(C)] pub struct SsymFollower { _p: [u8; 0] }

pub const SSYM_ABI_VERSION: i32 = 3;

pub const SSYM_OK: i32 = 0;
pub const SSYM_E_INVALID: i32 = -1;
pub const SSYM_E_EMPTY_DICT: i32 = -2;   // the panic at src/sound.rs:369
pub const SSYM_E_NO_DEVICE: i32 = -3;
pub const SSYM_E_HIP: i32 = -4;
pub const SSYM_E_NOMEM: i32 = -5;
pub const SSYM_E_UNSUPPORTED: i32 = -6;
pub const SSYM_E_TIMEOUT: i32 = -7;      // a rank of the sharded match did not arrive; the communicator is aborted
pub const SSYM_E_COMM: i32 = -8;         // the communicator is dead: destroy it

pub const SSYM_METRIC_REFCOS: i32 = 0;   // the crate's own cosine_sim / at_distance, bit for bit
pub const SSYM_METRIC_DTW: i32 = 1;
pub const SSYM_DTYPE_F64: i32 = 0;       // Sound::mfccs() is Vec<f64>
pub const SSYM_DTYPE_F32: i32 = 1;

pub const SSYM_OUT_DEVICE: u32 = 1;
pub const SSYM_WARP_MAP_DEVICE: u32 = 32;
pub const SSYM_FOLLOW_SAMPLES_DEVICE: u32 = 64;   // ssym_follow_envelope: `samples` is device memory
pub const SSYM_FOLLOW_REF_DEVICE: u32 = 128;      // ... and `ref`
pub const SSYM_DTW_FORCE_EXACT: u32 = 2;
pub const SSYM_DTW_PRUNE: u32 = 4;
pub const SSYM_STEP_SYMMETRIC: u32 = 0;  // the recurrence of ssym_dtw_spot: the _step calls are then the plain ones
pub const SSYM_STEP_PACED: u32 = 1;      // one source frame per target frame, at most one skipped or repeated in a row
pub const SSYM_MFCC_PAD_TAIL: u32 = 4;
pub const SSYM_TOPK_MAX: u32 = 64;
pub const SSYM_GMM_STANDARDIZE: u32 = 8;
pub const SSYM_PITCH_VOICED: u32 = 16;
pub const SSYM_PITCH_WINDOW: u64 = 2048;
pub const SSYM_PITCH_HOP: u64 = 1024;
pub const SSYM_NO_MATCH: u32 = 0xffff_ffff;
pub const SSYM_COVER_GAP: u32 = 0xffff_fffe;
pub const SSYM_COMM_ID_BYTES: usize = 128;

#[repr(C)]
pub struct SsymConfig {
    pub struct_size: u32,
    pub device: i32,
    pub metric: i32,
    pub dtype: i32,
    pub band: i32,         // dtw only, -1 = none
    pub dtw_squared: i32,
    pub stream: *mut c_void,
    pub dtw_prune: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct SsymTimings {
    pub pack_ms: f32,
    pub main_ms: f32,
    pub select_ms: f32,
    pub refine_ms: f32,
    pub reduce_ms: f32,
    pub total_ms: f32,
    pub n_pairs: u64,
    pub n_refined: u64,
    pub main_launches: i32,
    pub used_filter: i32,
    pub prune_ms: f32,
    pub pruned: i32,
    pub n_filter_cells: u64,
    pub collective_ms: f32,
    pub attempts: i32,
    pub exact_redone: i32,
    pub refcos_filter: i32,
}

extern "C" {
    pub fn ssym_abi_version() -> i32;
    pub fn ssym_ctx_create(cfg: *const SsymConfig, out: *mut *mut SsymCtx) -> i32;
    pub fn ssym_ctx_destroy(ctx: *mut SsymCtx) -> i32;
    pub fn ssym_last_error(ctx: *const SsymCtx) -> *const c_char;
    pub fn ssym_ctx_synchronize(ctx: *mut SsymCtx) -> i32;
    pub fn ssym_get_timings(ctx: *const SsymCtx, out: *mut SsymTimings) -> i32;

    pub fn ssym_dict_create(ctx: *mut SsymCtx, feats: *const c_void, frame_offsets: *const u64,
                            n_segments: u32, dim: u32, out: *mut *mut SsymDict) -> i32;
    pub fn ssym_dict_create_device(ctx: *mut SsymCtx, feats_dev: *const c_void, frame_offsets: *const u64,
                                   n_segments: u32, dim: u32, out: *mut *mut SsymDict) -> i32;
    pub fn ssym_dict_append(ctx: *mut SsymCtx, dict: *mut SsymDict, feats: *const c_void,
                            frame_offsets: *const u64, n_segments: u32) -> i32;
    pub fn ssym_dict_size(dict: *const SsymDict, out_n_segments: *mut u32) -> i32;
    pub fn ssym_dict_destroy(ctx: *mut SsymCtx, dict: *mut SsymDict) -> i32;

    pub fn ssym_queries_create(ctx: *mut SsymCtx, feats: *const c_void, frame_offsets: *const u64,
                               n_targets: u32, dim: u32, out: *mut *mut SsymQueries) -> i32;
    pub fn ssym_queries_create_device(ctx: *mut SsymCtx, feats_dev: *const c_void, frame_offsets: *const u64,
                                      n_targets: u32, dim: u32, out: *mut *mut SsymQueries) -> i32;
    pub fn ssym_queries_destroy(ctx: *mut SsymCtx, q: *mut SsymQueries) -> i32;

    pub fn ssym_match_queries(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, distance: *const f64,
                              index_base: u32, out_idx: *mut u32, out_cost: *mut f64, flags: u32) -> i32;
    pub fn ssym_match_topk(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, distance: *const f64,
                           k: u32, index_base: u32, out_idx: *mut u32, out_cost: *mut f64, flags: u32) -> i32;
    pub fn ssym_match_batch(ctx: *mut SsymCtx, dict: *const SsymDict, tgt_feats: *const c_void,
                            tgt_frame_offsets: *const u64, n_targets: u32, distance: *const f64,
                            out_idx: *mut u32, out_cost: *mut f64) -> i32;
    pub fn ssym_match_one(ctx: *mut SsymCtx, dict: *const SsymDict, feats: *const c_void, n_frames: u64,
                          distance: f64, out_idx: *mut u32, out_cost: *mut f64) -> i32;
    pub fn ssym_chain(ctx: *mut SsymCtx, dict: *mut SsymDict, start_feats: *const c_void, start_frames: u64,
                      distances: *const f64, n_steps: u32, out_idx: *mut u32, out_cost: *mut f64) -> i32;
    pub fn ssym_pair_matrix(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, exact: i32,
                            out_matrix: *mut f64) -> i32;
    // DTW alignment of listed pairs (dtw contexts): warping paths, costs, target-frame -> source-frame maps
    pub fn ssym_dtw_align_sizes(dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32, tgt_idx: *const u32,
                                n_pairs: u32, index_base: u32, path_offsets: *mut u64, map_offsets: *mut u64) -> i32;
    pub fn ssym_dtw_align(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                          tgt_idx: *const u32, n_pairs: u32, index_base: u32, out_cost: *mut f64, out_len: *mut u32,
                          path_offsets: *const u64, out_path: *mut u32, map_offsets: *const u64, out_map: *mut u32,
                          flags: u32) -> i32;
    // DTW spotting (subsequence DTW; dtw contexts without a band): the span of a dictionary segment's frames a target
    // aligns with best and its cost, per listed pair / the best segment per target; no spot: +inf and SSYM_NO_MATCH
    pub fn ssym_dtw_spot(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                         tgt_idx: *const u32, n_pairs: u32, index_base: u32, out_cost: *mut f64, out_start: *mut u32,
                         out_end: *mut u32, flags: u32) -> i32;
    pub fn ssym_spot_queries(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, index_base: u32,
                             out_idx: *mut u32, out_cost: *mut f64, out_start: *mut u32, out_end: *mut u32,
                             flags: u32) -> i32;
    // occurrences: up to max_spots (1 ... 64) pairwise disjoint spans per listed pair, best first, [n_pairs][max_spots]
    // row-major; max_cost: n_pairs thresholds in host memory or null; slots beyond out_count[p]: +inf and SSYM_NO_MATCH
    pub fn ssym_dtw_spot_all(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                             tgt_idx: *const u32, n_pairs: u32, index_base: u32, max_spots: u32, max_cost: *const f64,
                             out_count: *mut u32, out_cost: *mut f64, out_start: *mut u32, out_end: *mut u32,
                             flags: u32) -> i32;
    // the three calls above with a step pattern: SSYM_STEP_PACED bounds the slope (spans of about Fb / 2 to 2 Fb - 1 frames)
    // and makes cost / Fb a mean per-frame distance; targets of at most 2048 frames; costs and max_cost stay sums
    pub fn ssym_dtw_spot_step(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                              tgt_idx: *const u32, n_pairs: u32, index_base: u32, step: u32, out_cost: *mut f64,
                              out_start: *mut u32, out_end: *mut u32, flags: u32) -> i32;
    pub fn ssym_spot_queries_step(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, index_base: u32,
                                  step: u32, out_idx: *mut u32, out_cost: *mut f64, out_start: *mut u32,
                                  out_end: *mut u32, flags: u32) -> i32;
    pub fn ssym_dtw_spot_all_step(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                                  tgt_idx: *const u32, n_pairs: u32, index_base: u32, step: u32, max_spots: u32,
                                  max_cost: *const f64, out_count: *mut u32, out_cost: *mut f64, out_start: *mut u32,
                                  out_end: *mut u32, flags: u32) -> i32;
    // ssym_dtw_align with a step pattern: SSYM_STEP_PACED gives the path of the paced pattern between pinned ends (one cell
    // per target frame: out_len = Fb, or 0 without a finite cost); targets of at most 2048, sources of at most 4096 frames
    pub fn ssym_dtw_align_step(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                               tgt_idx: *const u32, n_pairs: u32, index_base: u32, step: u32, out_cost: *mut f64,
                               out_len: *mut u32, path_offsets: *const u64, out_path: *mut u32, map_offsets: *const u64,
                               out_map: *mut u32, flags: u32) -> i32;
    // ssym_dtw_align / ssym_dtw_align_step with a span of source frames per pair (span_first ..= span_last inside segment
    // src_idx[p] - index_base, HOST): what the spot calls report, aligned where it lies; cells and maps count from the span
    pub fn ssym_dtw_align_spans_sizes(dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32, tgt_idx: *const u32,
                                      span_first: *const u32, span_last: *const u32, n_pairs: u32, index_base: u32,
                                      path_offsets: *mut u64, map_offsets: *mut u64) -> i32;
    pub fn ssym_dtw_align_spans(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, src_idx: *const u32,
                                tgt_idx: *const u32, span_first: *const u32, span_last: *const u32, n_pairs: u32,
                                index_base: u32, step: u32, out_cost: *mut f64, out_len: *mut u32, path_offsets: *const u64,
                                out_path: *mut u32, map_offsets: *const u64, out_map: *mut u32, flags: u32) -> i32;
    // ssym_match_queries / ssym_pair_matrix with a step pattern: SSYM_STEP_PACED searches under the paced pattern (the cost of
    // a pair is ssym_dtw_align_step's paced cost, +inf without a paced shape; costs are sums over the target's frames)
    pub fn ssym_match_queries_step(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, distance: *const f64,
                                   index_base: u32, step: u32, out_idx: *mut u32, out_cost: *mut f64, flags: u32) -> i32;
    pub fn ssym_pair_matrix_step(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, step: u32,
                                 out_matrix: *mut f64) -> i32;
    // the cover: every target tiled by dictionary segments, cut points and segments chosen together for the least total of
    // paced costs (+ piece_penalty per piece); the four piece arrays hold one slot per target frame of the query set, target
    // t's pieces from slot frame_offset[t] on, unused slots SSYM_NO_MATCH / +inf; segments of at most 128 frames
    pub fn ssym_dtw_cover(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, piece_penalty: f64, flags: u32,
                          out_count: *mut u32, out_total: *mut f64, out_src: *mut u32, out_start: *mut u32,
                          out_end: *mut u32, out_cost: *mut f64) -> i32;
    // ... with target frames left uncovered at gap_cost per frame ("Cover with gaps"): a gap frame is the piece
    // (SSYM_COVER_GAP = 0xFFFFFFFE, e, e, gap_cost), one slot per frame; gap_cost = +inf is ssym_dtw_cover
    pub fn ssym_dtw_cover_gaps(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, piece_penalty: f64,
                               gap_cost: f64, flags: u32, out_count: *mut u32, out_total: *mut f64, out_src: *mut u32,
                               out_start: *mut u32, out_end: *mut u32, out_cost: *mut f64) -> i32;
    // the mosaic: every target tiled by free spans of dictionary segments of any length under the paced pattern, cuts,
    // segments, spans and paths chosen together; out_start lists a target's piece and gap-frame starts from slot
    // frame_offset[t] on (unused: SSYM_NO_MATCH), out_src / out_frame / out_frame_cost hold one entry per target frame
    // (a gap frame: SSYM_COVER_GAP, SSYM_NO_MATCH, gap_cost); every output may be null
    pub fn ssym_dtw_mosaic(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, piece_penalty: f64,
                           gap_cost: f64, flags: u32, out_count: *mut u32, out_total: *mut f64, out_start: *mut u32,
                           out_src: *mut u32, out_frame: *mut u32, out_frame_cost: *mut f64) -> i32;

    // source-sharded runs, exchange done by the caller (device pointers): filter / all-reduce(MIN) / finish / merge
    pub fn ssym_match_begin(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, distance: *const f64,
                            index_base: u32, bounds_dev: *mut f64) -> i32;
    pub fn ssym_match_finish(ctx: *mut SsymCtx, bounds_dev: *const f64, out_idx: *mut u32, out_cost: *mut f64,
                             flags: u32) -> i32;
    pub fn ssym_match_candidates(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries,
                                 cost_dev: *mut f64) -> i32;
    pub fn ssym_match_begin_pruned(ctx: *mut SsymCtx, dict: *const SsymDict, q: *const SsymQueries, index_base: u32,
                                   cost_dev: *const f64, bounds_dev: *mut f64) -> i32;
    pub fn ssym_merge_shards(ctx: *mut SsymCtx, n_shards: u32, n_targets: u32, costs_dev: *const f64,
                             idx_dev: *const u32, out_idx_dev: *mut u32, out_cost_dev: *mut f64) -> i32;
    pub fn ssym_merge_shards_at(ctx: *mut SsymCtx, n_shards: u32, n_targets: u32, costs_dev: *const f64,
                                idx_dev: *const u32, distance: *const f64, out_idx_dev: *mut u32,
                                out_cost_dev: *mut f64) -> i32;

    // source-sharded runs, exchange done by the library: RCCL on the context's stream, one host sync per step
    pub fn ssym_comm_unique_id(out_id: *mut c_void /* SSYM_COMM_ID_BYTES */) -> i32;
    pub fn ssym_comm_create(ctx: *mut SsymCtx, id: *const c_void, rank: i32, world: i32, out: *mut *mut SsymComm) -> i32;
    pub fn ssym_comm_destroy(ctx: *mut SsymCtx, comm: *mut SsymComm) -> i32;
    pub fn ssym_match_sharded(ctx: *mut SsymCtx, comm: *mut SsymComm, dict: *const SsymDict, q: *const SsymQueries,
                              distance: *const f64, index_base: u32, out_idx: *mut u32, out_cost: *mut f64,
                              flags: u32) -> i32;

    // the ranks of ONE process (a thread per rank) without RCCL: host barriers around device copies -- what the
    // one-GPU tests use to run more than one rank (RCCL refuses two ranks on one device)
    pub fn ssym_comm_available() -> i32;
    pub fn ssym_comm_set_timeout(comm: *mut SsymComm, milliseconds: i64) -> i32;
    pub fn ssym_comm_is_dead(comm: *const SsymComm) -> i32;
    // test and measurement hooks: refuse (SSYM_E_UNSUPPORTED) unless the process runs with SSYM_TEST_HOOKS=1
    pub fn ssym_comm_inject_fault(comm: *mut SsymComm, phase: i32, kind: i32) -> i32;
    pub fn ssym_comm_replay_bounds(comm: *mut SsymComm, bounds_dev: *const f64, n: u32) -> i32;
    pub fn ssym_local_group_create(world: i32, out: *mut *mut SsymLocalGroup) -> i32;
    pub fn ssym_local_group_destroy(group: *mut SsymLocalGroup) -> i32;
    pub fn ssym_comm_create_local(ctx: *mut SsymCtx, group: *mut SsymLocalGroup, rank: i32, out: *mut *mut SsymComm) -> i32;

    // reconstruction tail (src/sound.rs:456-465, 475-480, 139)
    pub fn ssym_samples_create(ctx: *mut SsymCtx, samples: *const f64, sample_offsets: *const u64, n_sounds: u32,
                               out: *mut *mut SsymSamples) -> i32;
    pub fn ssym_samples_destroy(ctx: *mut SsymCtx, s: *mut SsymSamples) -> i32;
    pub fn ssym_reconstruct(ctx: *mut SsymCtx, s: *const SsymSamples, idx: *const u32, out_offsets: *const u64,
                            n_targets: u32, out_samples: *mut f64, out_pcm32: *mut i32) -> i32;
    // warped reconstruction: every match resynthesised along ssym_dtw_align's target-frame -> source-frame map
    // (overlap-add of Hann-windowed source frames); flags: SSYM_OUT_DEVICE, SSYM_WARP_MAP_DEVICE (frame_map and pair_len
    // are device memory: ssym_dtw_align's device out_map / out_len pass straight in)
    pub fn ssym_reconstruct_warped(ctx: *mut SsymCtx, s: *const SsymSamples, idx: *const u32, out_offsets: *const u64,
                                   n_targets: u32, frame_map: *const u32, map_offsets: *const u64, map_frames: *const u32,
                                   pair_len: *const u32, flags: u32, out_samples: *mut f64, out_pcm32: *mut i32) -> i32;

    // WSOLA reconstruction: ssym_reconstruct_warped with every source frame moved by up to `search` (<= 512) samples to
    // where it continues the frame before it best; out_pos (nullable): the u64 sample start of every source frame, laid
    // out by map_offsets (device memory with SSYM_OUT_DEVICE)
    pub fn ssym_reconstruct_wsola(ctx: *mut SsymCtx, s: *const SsymSamples, idx: *const u32, out_offsets: *const u64,
                                  n_targets: u32, frame_map: *const u32, map_offsets: *const u64, map_frames: *const u32,
                                  pair_len: *const u32, search: u32, flags: u32, out_pos: *mut u64, out_samples: *mut f64,
                                  out_pcm32: *mut i32) -> i32;
    // the two calls above with a window of samples per target (win_first, win_len: HOST, in samples): sound idx[t] is only
    // that window, and the map counts frames from its start -- what ssym_dtw_align_spans returns
    pub fn ssym_reconstruct_warped_spans(ctx: *mut SsymCtx, s: *const SsymSamples, idx: *const u32, win_first: *const u64,
                                         win_len: *const u64, out_offsets: *const u64, n_targets: u32, frame_map: *const u32,
                                         map_offsets: *const u64, map_frames: *const u32, pair_len: *const u32, flags: u32,
                                         out_samples: *mut f64, out_pcm32: *mut i32) -> i32;
    pub fn ssym_reconstruct_wsola_spans(ctx: *mut SsymCtx, s: *const SsymSamples, idx: *const u32, win_first: *const u64,
                                        win_len: *const u64, out_offsets: *const u64, n_targets: u32, frame_map: *const u32,
                                        map_offsets: *const u64, map_frames: *const u32, pair_len: *const u32, search: u32,
                                        flags: u32, out_pos: *mut u64, out_samples: *mut f64, out_pcm32: *mut i32) -> i32;

    // envelope following: reconstructions (packed by out_offsets) scaled hop by hop to the loudness of their references
    // (packed by ref_offsets), no gain above max_gain; out_gain (nullable): g(b) of all targets packed in target order.
    // flags: SSYM_FOLLOW_SAMPLES_DEVICE, SSYM_FOLLOW_REF_DEVICE, SSYM_OUT_DEVICE (the three outputs).  Any context
    pub fn ssym_follow_envelope(ctx: *mut SsymCtx, samples: *const f64, out_offsets: *const u64, n_targets: u32,
                                reference: *const f64, ref_offsets: *const u64, max_gain: f64, flags: u32,
                                out_samples: *mut f64, out_pcm32: *mut i32, out_gain: *mut f64) -> i32;

    // feature front-end (own MFCC definition -- parity with vox_box unpinned)
    pub fn ssym_mfcc_num_frames(n_samples: u64, flags: u32, out_frames: *mut u64) -> i32;
    pub fn ssym_mfcc(ctx: *mut SsymCtx, samples: *const f64, n_samples: u64, sample_rate: f64, n_coeffs: u32,
                     f_lo: f64, f_hi: f64, flags: u32, out_mfccs: *mut f64, out_mean: *mut f64) -> i32;
    pub fn ssym_mfcc_batch(ctx: *mut SsymCtx, samples: *const f64, sample_offsets: *const u64, n_sounds: u32,
                           sample_rate: f64, n_coeffs: u32, f_lo: f64, f_hi: f64, flags: u32,
                           out_frame_offsets: *mut u64, out_mfccs: *mut f64, out_mean: *mut f64) -> i32;
    // SoundSequence::new's neighbour distances (mean MFCCs, cosine_sim_angular)
    pub fn ssym_sequence_distances(ctx: *mut SsymCtx, feats: *const f64, frame_offsets: *const u64, n_sounds: u32,
                                   dim: u32, flags: u32, out_mean: *mut f64, out_sim: *mut f64,
                                   out_dist: *mut f64) -> i32;

    // partitioner: standardiser, Gaussian mixture, voting experts (own definitions -- parity unpinned)
    pub fn ssym_standardize(ctx: *mut SsymCtx, feats: *const f64, n_frames: u64, dim: u32, flags: u32,
                            out: *mut f64) -> i32;
    pub fn ssym_gmm_train(ctx: *mut SsymCtx, feats: *const f64, n_frames: u64, dim: u32, n_components: u32,
                          init_rows: *const u64, eps: f64, max_iters: u32, flags: u32, out: *mut *mut SsymGmm) -> i32;
    pub fn ssym_gmm_get(gmm: *const SsymGmm, weights: *mut f64, means: *mut f64, covs: *mut f64, log_lik: *mut f64,
                        iters: *mut u32) -> i32;
    pub fn ssym_gmm_destroy(ctx: *mut SsymCtx, gmm: *mut SsymGmm) -> i32;
    pub fn ssym_gmm_predict(ctx: *mut SsymCtx, gmm: *const SsymGmm, feats: *const f64, n_frames: u64, flags: u32,
                            out_post: *mut f64, out_letters: *mut u8) -> i32;
    pub fn ssym_vote_segments(ctx: *mut SsymCtx, symbols: *const u8, n: u64, alphabet: u32, depth: u32, threshold: u32,
                              flags: u32, out_votes: *mut u32, out_seg_frames: *mut u64, n_segments: *mut u64) -> i32;
    pub fn ssym_partition(ctx: *mut SsymCtx, gmm: *const SsymGmm, feats: *const f64, n_frames: u64, depth: u32,
                          threshold: u32, flags: u32, out_seg_frames: *mut u64, n_segments: *mut u64) -> i32;

    // sound descriptors: max_power and pitch_confidence of a ragged batch (pitch: own definition -- parity unpinned)
    pub fn ssym_pitch_num_windows(n_samples: u64, out_windows: *mut u64) -> i32;
    pub fn ssym_sound_descriptors(ctx: *mut SsymCtx, samples: *const f64, sample_offsets: *const u64, n_sounds: u32,
                                  rate: f64, f_min: f64, f_max: f64, voicing: f64, flags: u32,
                                  out_max_power: *mut f64, out_pitch_conf: *mut f64) -> i32;
    pub fn ssym_pitch_track(ctx: *mut SsymCtx, samples: *const f64, sample_offsets: *const u64, n_sounds: u32,
                            rate: f64, f_min: f64, f_max: f64, voicing: f64, flags: u32, out_freq: *mut f64,
                            out_strength: *mut f64, out_unvoiced: *mut f64) -> i32;

    // streaming sounds: Sound::push_samples (src/sound.rs:145-164) with samples and analysis resident on the device
    pub fn ssym_stream_create(ctx: *mut SsymCtx, n_lanes: u32, sample_rate: f64, n_coeffs: u32, f_lo: f64, f_hi: f64,
                              capacity_hint_samples: u64, out: *mut *mut SsymStream) -> i32;
    pub fn ssym_stream_destroy(ctx: *mut SsymCtx, st: *mut SsymStream) -> i32;
    pub fn ssym_stream_push(ctx: *mut SsymCtx, st: *mut SsymStream, samples: *const f64, sample_offsets: *const u64,
                            flags: u32, out_new_frames: *mut u64, out_mfccs: *mut f64) -> i32;
    pub fn ssym_stream_seed(ctx: *mut SsymCtx, st: *mut SsymStream, lane: u32, samples: *const f64, n_samples: u64,
                            mfccs: *const f64, n_frames: u64) -> i32;
    pub fn ssym_stream_counts(st: *const SsymStream, out_n_samples: *mut u64, out_n_frames: *mut u64) -> i32;
    pub fn ssym_stream_read(ctx: *mut SsymCtx, st: *mut SsymStream, lane: u32, first_frame: u64, n_frames: u64,
                            flags: u32, out_mfccs: *mut f64) -> i32;
    pub fn ssym_stream_frames_device(st: *const SsymStream, lane: u32, out_ptr: *mut *const f64,
                                     out_n_frames: *mut u64) -> i32;
    pub fn ssym_stream_samples_device(st: *const SsymStream, lane: u32, out_ptr: *mut *const f64,
                                      out_n_samples: *mut u64) -> i32;
    pub fn ssym_stream_descriptors(ctx: *mut SsymCtx, st: *mut SsymStream, out_max_power: *mut f64,
                                   out_mean: *mut f64) -> i32;
    pub fn ssym_stream_reset(ctx: *mut SsymCtx, st: *mut SsymStream, lane: u32) -> i32;

    // watching: the targets of a query set spotted in growing sources, resumable push by push
    pub fn ssym_spotter_create(ctx: *mut SsymCtx, q: *const SsymQueries, n_lanes: u32, max_cost: *const f64,
                               out: *mut *mut SsymSpotter) -> i32;
    pub fn ssym_spotter_destroy(ctx: *mut SsymCtx, sp: *mut SsymSpotter) -> i32;
    pub fn ssym_spotter_push(ctx: *mut SsymCtx, sp: *mut SsymSpotter, feats: *const f64, frame_offsets: *const u64,
                             flags: u32, out_n_events: *mut u64, out_profile_cost: *mut f64,
                             out_profile_start: *mut u32) -> i32;
    pub fn ssym_spotter_follow(ctx: *mut SsymCtx, sp: *mut SsymSpotter, stream: *const SsymStream, flags: u32,
                               out_n_events: *mut u64, out_profile_cost: *mut f64, out_profile_start: *mut u32) -> i32;
    pub fn ssym_spotter_events(ctx: *mut SsymCtx, sp: *const SsymSpotter, out_lane: *mut u32, out_target: *mut u32,
                               out_cost: *mut f64, out_start: *mut u32, out_end: *mut u32, flags: u32) -> i32;
    pub fn ssym_spotter_flush(ctx: *mut SsymCtx, sp: *mut SsymSpotter, lane: u32, out_n_events: *mut u64) -> i32;
    pub fn ssym_spotter_best(ctx: *mut SsymCtx, sp: *const SsymSpotter, out_cost: *mut f64, out_start: *mut u32,
                             out_end: *mut u32, flags: u32) -> i32;
    pub fn ssym_spotter_counts(sp: *const SsymSpotter, out_frames: *mut u64) -> i32;
    pub fn ssym_spotter_reset(ctx: *mut SsymCtx, sp: *mut SsymSpotter, lane: u32) -> i32;
    // ssym_spotter_create with a step pattern: under SSYM_STEP_PACED the spotter's spans keep the paced slope bounds, a NaN
    // frame costs a bounded stretch of a lane, and the state is two rows per (lane, target); max_cost stays a sum
    pub fn ssym_spotter_create_step(ctx: *mut SsymCtx, q: *const SsymQueries, n_lanes: u32, max_cost: *const f64,
                                    step: u32, out: *mut *mut SsymSpotter) -> i32;
    // the live cover ("Live cover" in soundsym_amd.h): growing targets tiled by the segments of one resident dictionary, every
    // piece reported by the push after which no longer recording could change it; the dictionary must outlive the coverer
    pub fn ssym_coverer_create(ctx: *mut SsymCtx, dict: *const SsymDict, n_lanes: u32, piece_penalty: f64,
                               out: *mut *mut SsymCoverer) -> i32;
    // ... with gaps: a NaN or +-inf frame becomes a gap frame and the lane goes on; every other call works on it unchanged
    pub fn ssym_coverer_create_gaps(ctx: *mut SsymCtx, dict: *const SsymDict, n_lanes: u32, piece_penalty: f64, gap_cost: f64,
                                    out: *mut *mut SsymCoverer) -> i32;
    pub fn ssym_coverer_destroy(ctx: *mut SsymCtx, cv: *mut SsymCoverer) -> i32;
    pub fn ssym_coverer_push(ctx: *mut SsymCtx, cv: *mut SsymCoverer, feats: *const f64, frame_offsets: *const u64,
                             flags: u32, out_n_pieces: *mut u64) -> i32;
    pub fn ssym_coverer_follow(ctx: *mut SsymCtx, cv: *mut SsymCoverer, stream: *const SsymStream, flags: u32,
                               out_n_pieces: *mut u64) -> i32;
    pub fn ssym_coverer_pieces(ctx: *mut SsymCtx, cv: *const SsymCoverer, out_lane: *mut u32, out_src: *mut u32,
                               out_start: *mut u32, out_end: *mut u32, out_cost: *mut f64, flags: u32) -> i32;
    pub fn ssym_coverer_flush(ctx: *mut SsymCtx, cv: *mut SsymCoverer, lane: u32, out_n_pieces: *mut u64) -> i32;
    pub fn ssym_coverer_best(ctx: *mut SsymCtx, cv: *const SsymCoverer, out_total: *mut f64, out_covered: *mut u32,
                             out_committed: *mut u32, flags: u32) -> i32;
    pub fn ssym_coverer_counts(cv: *const SsymCoverer, out_frames: *mut u64, out_capacity: *mut u64) -> i32;
    pub fn ssym_coverer_reset(ctx: *mut SsymCtx, cv: *mut SsymCoverer, lane: u32) -> i32;
    // live mosaic ("Live mosaic"): n_lanes growing targets tiled by free spans of the recordings of one resident dictionary,
    // every target frame reported by the push after which no longer recording could change it; gap_cost +inf: no gaps; the
    // dictionary must outlive the mosaicker
    pub fn ssym_mosaicker_create(ctx: *mut SsymCtx, dict: *const SsymDict, n_lanes: u32, piece_penalty: f64, gap_cost: f64,
                                 out: *mut *mut SsymMosaicker) -> i32;
    pub fn ssym_mosaicker_destroy(ctx: *mut SsymCtx, mk: *mut SsymMosaicker) -> i32;
    pub fn ssym_mosaicker_push(ctx: *mut SsymCtx, mk: *mut SsymMosaicker, feats: *const f64, frame_offsets: *const u64,
                               flags: u32, out_n_frames: *mut u64) -> i32;
    pub fn ssym_mosaicker_follow(ctx: *mut SsymCtx, mk: *mut SsymMosaicker, stream: *const SsymStream, flags: u32,
                                 out_n_frames: *mut u64) -> i32;
    pub fn ssym_mosaicker_frames(ctx: *mut SsymCtx, mk: *const SsymMosaicker, out_lane: *mut u32, out_column: *mut u32,
                                 out_src: *mut u32, out_frame: *mut u32, out_cost: *mut f64, out_start: *mut u32,
                                 flags: u32) -> i32;
    pub fn ssym_mosaicker_flush(ctx: *mut SsymCtx, mk: *mut SsymMosaicker, lane: u32, out_n_frames: *mut u64) -> i32;
    pub fn ssym_mosaicker_best(ctx: *mut SsymCtx, mk: *const SsymMosaicker, out_total: *mut f64, out_covered: *mut u32,
                               out_committed: *mut u32, flags: u32) -> i32;
    pub fn ssym_mosaicker_counts(mk: *const SsymMosaicker, out_frames: *mut u64, out_capacity: *mut u64) -> i32;
    pub fn ssym_mosaicker_reset(ctx: *mut SsymCtx, mk: *mut SsymMosaicker, lane: u32) -> i32;
    // live resynthesis (include/soundsym_amd.h "Live resynthesis"): committed mosaic frames to audio, push by push; the
    // sample store must outlive the resynthesiser
    pub fn ssym_resynth_create(ctx: *mut SsymCtx, store: *const SsymSamples, n_lanes: u32, search: u32,
                               out: *mut *mut SsymResynth) -> i32;
    pub fn ssym_resynth_destroy(ctx: *mut SsymCtx, rs: *mut SsymResynth) -> i32;
    pub fn ssym_resynth_push(ctx: *mut SsymCtx, rs: *mut SsymResynth, lane: *const u32, column: *const u32, src: *const u32,
                             frame: *const u32, start: *const u32, n_frames: u64, out_n_samples: *mut u64) -> i32;
    pub fn ssym_resynth_take(ctx: *mut SsymCtx, rs: *mut SsymResynth, mk: *const SsymMosaicker, out_n_samples: *mut u64) -> i32;
    pub fn ssym_resynth_samples(ctx: *mut SsymCtx, rs: *const SsymResynth, out_lane_offsets: *mut u64, out_samples: *mut f64,
                                out_pcm32: *mut i32, flags: u32) -> i32;
    pub fn ssym_resynth_flush(ctx: *mut SsymCtx, rs: *mut SsymResynth, lane: u32, total_samples: u64,
                              out_n_samples: *mut u64) -> i32;
    pub fn ssym_resynth_counts(rs: *const SsymResynth, out_frames: *mut u64, out_samples: *mut u64) -> i32;
    pub fn ssym_resynth_reset(ctx: *mut SsymCtx, rs: *mut SsymResynth, lane: u32) -> i32;
    // live envelope following (include/soundsym_amd.h "Live envelope following"): loudness tracking, push by push; samples and
    // ref are host memory, or device memory with SSYM_FOLLOW_SAMPLES_DEVICE / SSYM_FOLLOW_REF_DEVICE
    pub fn ssym_follower_create(ctx: *mut SsymCtx, n_lanes: u32, max_gain: f64, out: *mut *mut SsymFollower) -> i32;
    pub fn ssym_follower_destroy(ctx: *mut SsymCtx, fl: *mut SsymFollower) -> i32;
    pub fn ssym_follower_push(ctx: *mut SsymCtx, fl: *mut SsymFollower, samples: *const f64, sample_offsets: *const u64,
                              reference: *const f64, ref_offsets: *const u64, flags: u32, out_n_samples: *mut u64) -> i32;
    pub fn ssym_follower_flush(ctx: *mut SsymCtx, fl: *mut SsymFollower, lane: u32, out_n_samples: *mut u64) -> i32;
    pub fn ssym_follower_samples(ctx: *mut SsymCtx, fl: *const SsymFollower, out_lane_offsets: *mut u64, out_samples: *mut f64,
                                 out_pcm32: *mut i32, out_gain_offsets: *mut u64, out_gain: *mut f64, flags: u32) -> i32;
    pub fn ssym_follower_counts(fl: *const SsymFollower, out_ny: *mut u64, out_nx: *mut u64, out_released: *mut u64) -> i32;
    pub fn ssym_follower_reset(ctx: *mut SsymCtx, fl: *mut SsymFollower, lane: u32) -> i32;
}

/// `Err(message)` for any status but SSYM_OK; SSYM_E_EMPTY_DICT keeps the crate's behaviour (a panic, :369).
pub unsafe fn check(ctx: *const SsymCtx, rc: i32) -> Result<(), String> {
    if rc == SSYM_OK {
        return Ok(());
    }
    if rc == SSYM_E_EMPTY_DICT {
        panic!("index out of bounds: the len is 0 but the index is 0");   // what src/sound.rs:369 does today
    }
    let msg = ssym_last_error(ctx);
    let text = if msg.is_null() { String::new() } else { std::ffi::CStr::from_ptr(msg).to_string_lossy().into_owned() };
    Err(format!("soundsym_amd error {}: {}", rc, text))
}
