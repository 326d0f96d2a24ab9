// soundsym.hpp -- C++ host mirror of the reference's matching interface over the C ABI.
//
// The reference is a compiled (Rust) crate and this image has no Rust toolchain, so the host side
// above `include/soundsym_amd.h` is C++ with the reference's names, argument meaning and error
// behaviour for the hot path (upstream src/sound.rs):
//
//   Sound::from_samples / samples / sample_rate / mfccs / num_frames     :92, :181-212
//   SoundDictionary::new_ / from_segments / add_segments                 :296, :323, :330
//   SoundDictionary::match_sound / at_distance                           :346, :351
//   SoundSequence::new_ / sounds / from_distances / morph_to /
//                  clone_from_dictionary / to_sound                      :392-483
//
// `Arc<Sound>` is `std::shared_ptr<const Sound>`; `Option<Arc<Sound>>` is returned as the pointer
// itself (the reference never returns None, :369); `Result<_, String>` becomes an exception of
// type soundsym::Error; the reference's panic on an empty dictionary (:369) becomes
// soundsym::EmptyDictionary.  Feature extraction (:215-242) is out of scope: a Sound is built from
// samples plus ready-made features (the `Some(mfccs)` form of from_samples, :92-94).
//
// Header-only; link libsoundsym_amd.so and one HIP runtime.
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <array>
#include <vector>

#include "soundsym_amd.h"

namespace soundsym {

constexpr std::size_t NCOEFFS = 12;   // src/lib.rs:22
constexpr std::size_t HOP = 256;      // src/lib.rs:24
constexpr std::size_t BIN = 1024;     // src/lib.rs:25

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct EmptyDictionary : Error {
    EmptyDictionary() : Error(SSYM_E_EMPTY_DICT, "empty dictionary (the reference panics here, src/sound.rs:369)") {}
};

// One GPU context; metric 0 = refcos (the crate's own cosine_sim), 1 = dtw.
class Context {
  public:
    // prune: dtw nearest-neighbour searches of 64 targets and more abandon pairs early (same results,
    // data-dependent time)
    explicit Context(int metric = SSYM_METRIC_REFCOS, int device = 0, int band = -1, bool squared = false,
                     bool prune = false)
    {
        ssym_config cfg{};
        cfg.struct_size = sizeof(cfg);
        cfg.device = device;
        cfg.metric = metric;
        cfg.dtype = SSYM_DTYPE_F64;   // Sound::mfccs() is Vec<f64>
        cfg.band = band;
        cfg.dtw_squared = squared ? 1 : 0;
        cfg.stream = nullptr;
        cfg.dtw_prune = prune ? 1 : 0;
        int rc = ssym_ctx_create(&cfg, &ctx_);
        if (rc != SSYM_OK)
            throw Error(rc, ssym_last_error(nullptr));
        metric_ = metric;
    }
    ~Context() { ssym_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ssym_ctx *get() const { return ctx_; }
    int metric() const { return metric_; }
    void check(int rc) const
    {
        if (rc == SSYM_E_EMPTY_DICT)
            throw EmptyDictionary();
        if (rc != SSYM_OK)
            throw Error(rc, ssym_last_error(ctx_));
    }

  private:
    ssym_ctx *ctx_ = nullptr;
    int metric_ = 0;
};

class Sound {
  public:
    std::optional<std::string> name;

    // Sound::from_samples(samples, sample_rate, mfccs, name), src/sound.rs:92
    static Sound from_samples(std::vector<double> samples, double sample_rate,
                              std::optional<std::vector<double>> mfccs, std::optional<std::string> name)
    {
        Sound s;
        s.samples_ = std::move(samples);
        s.sample_rate_ = sample_rate;
        if (mfccs) {
            if (mfccs->size() % NCOEFFS)
                throw Error(SSYM_E_INVALID, "mfccs must hold whole frames of NCOEFFS values");
            s.mfccs_ = std::move(*mfccs);
            s.has_mfccs_ = true;
        }
        s.name = std::move(name);
        return s;
    }
    // The `None` form of from_samples (src/sound.rs:97-101): run the MFCC analysis (analyze_mfccs,
    // :215-242) -- on the GPU, ssym_mfcc; its arithmetic is this library's own definition (parity
    // with the un-vendored vox_box MFCC is unpinned).
    template <class Ctx>
    static Sound from_samples(Ctx &ctx, std::vector<double> samples, double sample_rate,
                              std::optional<std::string> name = std::nullopt)
    {
        uint64_t frames = 0;
        ssym_mfcc_num_frames(samples.size(), 0, &frames);
        std::vector<double> m(frames * NCOEFFS);
        ctx.check(ssym_mfcc(ctx.get(), samples.data(), samples.size(), sample_rate, (uint32_t)NCOEFFS, 100.0,
                            8000.0, 0, m.data(), nullptr));
        return from_samples(std::move(samples), sample_rate, std::move(m), std::move(name));
    }
    const std::vector<double> &samples() const { return samples_; }   // :181
    double sample_rate() const { return sample_rate_; }                // :185
    const std::vector<double> &mfccs() const                           // :191
    {
        if (!has_mfccs_)
            throw Error(SSYM_E_INVALID, "this Sound carries no features (use the from_samples overload that analyses)");
        return mfccs_;
    }
    bool has_mfccs() const { return has_mfccs_; }
    std::size_t num_frames() const { return mfccs().size() / NCOEFFS; }   // :210

  private:
    std::vector<double> samples_, mfccs_;
    double sample_rate_ = 44100.0;
    bool has_mfccs_ = false;
};

using ArcSound = std::shared_ptr<const Sound>;

inline void pack_features(const std::vector<ArcSound> &sounds, std::vector<double> &flat,
                          std::vector<uint64_t> &off)
{
    off.assign(1, 0);
    flat.clear();
    for (const auto &s : sounds) {
        const auto &m = s->mfccs();
        flat.insert(flat.end(), m.begin(), m.end());
        off.push_back(off.back() + m.size() / NCOEFFS);
    }
}

// What a reconstruction does about loudness: None plays every matched span at the level it was recorded at, Target sends
// the result through follow_envelope against the targets' own samples.
enum class Dynamics { None, Target };

// Envelope following (ssym_follow_envelope; any context): the reconstructions `samples`, packed by out_offsets, scaled hop
// by hop to the loudness of the references `ref`, packed by ref_offsets -- a reference shorter than its reconstruction is
// silent from its end, what it has beyond the reconstruction's length is not used; no gain above max_gain (finite, at
// least 1).  Returns the samples; gains (nullable) receives g(b) of all targets packed in target order, ceil(n / 256) + 1
// per target of n > 0 samples.
inline std::vector<double> follow_envelope(const Context &ctx, const std::vector<double> &samples,
                                           const std::vector<uint64_t> &out_offsets, const std::vector<double> &ref,
                                           const std::vector<uint64_t> &ref_offsets, double max_gain = 8.0,
                                           std::vector<double> *gains = nullptr)
{
    if (out_offsets.empty() || ref_offsets.size() != out_offsets.size())
        throw Error(SSYM_E_INVALID, "follow_envelope: n + 1 out_offsets and n + 1 ref_offsets for n targets");
    if (samples.size() < out_offsets.back() || ref.size() < ref_offsets.back())
        throw Error(SSYM_E_INVALID, "follow_envelope: samples or ref hold fewer values than their offsets ask for");
    const uint32_t n = (uint32_t)(out_offsets.size() - 1);
    std::vector<double> out(out_offsets.back());
    if (gains) {
        std::size_t count = 0;
        for (uint32_t t = 0; t < n && out_offsets[t + 1] >= out_offsets[t]; ++t)
            if (const uint64_t len = out_offsets[t + 1] - out_offsets[t])
                count += (std::size_t)((len + SSYM_MFCC_HOP - 1) / SSYM_MFCC_HOP + 1);
        gains->assign(count, 0.0);
    }
    ctx.check(ssym_follow_envelope(ctx.get(), samples.data(), out_offsets.data(), n, ref.data(), ref_offsets.data(), max_gain, 0,
                                   out.empty() ? nullptr : out.data(), nullptr,
                                   gains && !gains->empty() ? gains->data() : nullptr));
    return out;
}

// the Dynamics::Target tail of the reconstructing methods: one follow_envelope call against the targets' own samples
template <class Targets>
inline std::vector<double> follow_targets(const Context &ctx, std::vector<double> out, const Targets &targets,
                                          const std::vector<uint64_t> &ooff, double max_gain)
{
    std::vector<double> ref;
    for (const auto &t : targets)
        ref.insert(ref.end(), t->samples().begin(), t->samples().end());
    return follow_envelope(ctx, out, ooff, ref, ooff, max_gain);
}

class SoundDictionary {
  public:
    std::vector<ArcSound> sounds;   // `pub sounds: Vec<Arc<Sound>>`, src/sound.rs:291

    explicit SoundDictionary(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
    ~SoundDictionary() { release(); }
    SoundDictionary(const SoundDictionary &) = delete;
    SoundDictionary &operator=(const SoundDictionary &) = delete;

    static std::unique_ptr<SoundDictionary> new_(std::shared_ptr<Context> ctx)   // :296
    {
        return std::make_unique<SoundDictionary>(std::move(ctx));
    }
    static std::unique_ptr<SoundDictionary> from_segments(std::shared_ptr<Context> ctx, const Sound &sound,
                                                          const std::vector<std::size_t> &segments)   // :323
    {
        auto d = new_(std::move(ctx));
        d->add_segments(sound, segments);
        return d;
    }
    // src/sound.rs:330-343: `seg` samples and `seg / HOP * NCOEFFS` feature values per segment,
    // consumed in order from the parent sound (`take` on an exhausted iterator yields what is left)
    void add_segments(const Sound &sound, const std::vector<std::size_t> &segments)
    {
        const auto &samples = sound.samples();
        const auto &mfccs = sound.mfccs();
        std::size_t spos = 0, mpos = 0;
        for (std::size_t seg : segments) {
            std::size_t se = std::min(spos + seg, samples.size());
            std::size_t nm = seg / HOP * NCOEFFS, me = std::min(mpos + nm, mfccs.size());
            std::vector<double> samp(samples.begin() + spos, samples.begin() + se);
            std::vector<double> mf(mfccs.begin() + mpos, mfccs.begin() + me);
            spos = se;
            mpos = me;
            sounds.push_back(std::make_shared<const Sound>(
                Sound::from_samples(std::move(samp), sound.sample_rate(), std::move(mf), std::nullopt)));
        }
    }

    ArcSound match_sound(const Sound &other) const   // :346  at_distance(1., other)
    {
        return at_distance(ctx_->metric() == SSYM_METRIC_REFCOS ? 1.0 : 0.0, other);
    }
    ArcSound at_distance(double distance, const Sound &other) const   // :351
    {
        if (sounds.empty())
            throw EmptyDictionary();
        uint32_t idx = 0;
        double val = 0.0;
        ctx_->check(ssym_match_one(ctx_->get(), resident(), other.mfccs().data(), other.num_frames(), distance,
                                   &idx, &val));
        return sounds[idx];   // Some(self.sounds[min_idx].clone())
    }
    // batched form of the loops at :442-446 and :453-454
    std::vector<uint32_t> match_indices(const std::vector<ArcSound> &targets, const double *distances) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        std::vector<uint32_t> idx(targets.size());
        ctx_->check(ssym_match_batch(ctx_->get(), resident(), flat.data(), off.data(), (uint32_t)targets.size(),
                                     distances, idx.data(), nullptr));
        return idx;
    }
    // match_indices under a step pattern (ssym_match_queries_step): SSYM_STEP_PACED searches under the paced pattern of
    // soundsym_amd.h "Paced matching" -- the cost of a pair is its paced alignment's (+inf where the shapes admit no paced
    // path), costs[t] (if asked for) the winner's, a sum over the target's frames; a target nothing fits gets 0 and +inf
    std::vector<uint32_t> match_indices_step(const std::vector<ArcSound> &targets, const double *distances, uint32_t step,
                                             std::vector<double> *costs = nullptr) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty()) {   // n_targets = 0 succeeds and does nothing (soundsym_amd.h); no NULL of an empty vector reaches the library
            if (costs)
                costs->clear();
            return {};
        }
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), (uint32_t)targets.size(),
                                        (uint32_t)NCOEFFS, &q));
        std::vector<uint32_t> idx(targets.size());
        if (costs)
            costs->assign(targets.size(), 0.0);
        int32_t rc = ssym_match_queries_step(ctx_->get(), resident(), q, distances, 0, step, idx.data(),
                                             costs ? costs->data() : nullptr, 0);
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        return idx;
    }
    // the [sounds][targets] costs of a step pattern (ssym_pair_matrix_step), row-major
    std::vector<double> pair_matrix_step(const std::vector<ArcSound> &targets, uint32_t step) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty())
            return {};
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), (uint32_t)targets.size(),
                                        (uint32_t)NCOEFFS, &q));
        std::vector<double> out(sounds.size() * targets.size());
        int32_t rc = ssym_pair_matrix_step(ctx_->get(), resident(), q, step, out.data());
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        return out;
    }

    // the k best sounds per target, best first (ssym_match_topk; the crate has no counterpart:
    // at_distance keeps only the first minimum, :361-367)
    std::vector<std::vector<ArcSound>> candidates(const std::vector<ArcSound> &targets, uint32_t k,
                                                  const double *distances = nullptr) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty())
            return {};
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), (uint32_t)targets.size(),
                                        (uint32_t)NCOEFFS, &q));
        std::vector<uint32_t> idx(targets.size() * k);
        int32_t rc = ssym_match_topk(ctx_->get(), resident(), q, distances, k, 0, idx.data(), nullptr, 0);
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        std::vector<std::vector<ArcSound>> out(targets.size());
        for (std::size_t t = 0; t < targets.size(); ++t)
            for (uint32_t r = 0; r < k; ++r)
                if (idx[t * k + r] != SSYM_NO_MATCH)
                    out[t].push_back(sounds[idx[t * k + r]]);
        return out;
    }
    // the warping path of every target onto dictionary sound indices[t] (ssym_dtw_align; dtw contexts; the crate has
    // no counterpart).  path: (source frame, target frame) cells in forward order; frame_map: the smallest source
    // frame aligned with every target frame; both empty for a pair without a finite cost
    struct Alignment {
        double cost;
        std::vector<std::array<uint32_t, 2>> path;
        std::vector<uint32_t> frame_map;
        uint32_t source_index;
    };
    // step: SSYM_STEP_SYMMETRIC (ssym_dtw_align) or SSYM_STEP_PACED (ssym_dtw_align_step; soundsym_amd.h "Paced
    // alignment": one cell per target frame, the alignment of a span a paced spot found)
    std::vector<Alignment> align(const std::vector<ArcSound> &targets, const std::vector<uint32_t> &indices,
                                 uint32_t step = SSYM_STEP_SYMMETRIC) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty() && indices.empty())
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), n, (uint32_t)NCOEFFS, &q));
        std::vector<uint64_t> poff(n + 1), moff(n + 1);
        std::vector<double> cost(n);
        std::vector<uint32_t> len(n), path, map;
        int32_t rc = indices.size() == n ? ssym_dtw_align_sizes(resident(), q, indices.data(), nullptr, n, 0, poff.data(),
                                                                moff.data())
                                         : (int32_t)SSYM_E_INVALID;
        if (rc == SSYM_OK) {
            path.resize(2 * poff[n]);
            map.resize(moff[n]);
            rc = step == SSYM_STEP_SYMMETRIC
                     ? ssym_dtw_align(ctx_->get(), resident(), q, indices.data(), nullptr, n, 0, cost.data(), len.data(),
                                      poff.data(), path.data(), moff.data(), map.data(), 0)
                     : ssym_dtw_align_step(ctx_->get(), resident(), q, indices.data(), nullptr, n, 0, step, cost.data(),
                                           len.data(), poff.data(), path.data(), moff.data(), map.data(), 0);
        }
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        std::vector<Alignment> out(n);
        for (uint32_t t = 0; t < n; ++t) {
            out[t].cost = cost[t];
            out[t].source_index = indices[t];
            for (uint32_t s = 0; s < len[t]; ++s)
                out[t].path.push_back({path[2 * (poff[t] + s)], path[2 * (poff[t] + s) + 1]});
            if (len[t])
                out[t].frame_map.assign(map.begin() + moff[t], map.begin() + moff[t + 1]);
        }
        return out;
    }
    // the reconstruction of the targets with dictionary sound indices[t] warped onto target t's timing: align, then
    // resynthesise along each frame_map (ssym_dtw_align + ssym_reconstruct_warped; dtw contexts; the crate has no
    // counterpart).  One stretch of targets[t]->samples().size() samples per target, concatenated; a pair without a
    // finite cost takes clone_from_dictionary's length fit.  (The mirror holds no device memory of its own, so the
    // maps pass through the host here; a caller with device buffers hands ssym_dtw_align's SSYM_OUT_DEVICE outputs
    // to ssym_reconstruct_warped with SSYM_WARP_MAP_DEVICE.)  search > 0 (at most 512 samples): ssym_reconstruct_wsola
    // instead -- every source frame may move that far to where it continues the frame before it in phase.
    // dynamics = Dynamics::Target: the result goes through one follow_envelope call against the targets' own samples
    // (max_gain as there, checked before anything else); Dynamics::None: the reconstruction as it is, no extra call.
    std::vector<double> warp(const std::vector<ArcSound> &targets, const std::vector<uint32_t> &indices,
                             uint32_t search = 0, Dynamics dynamics = Dynamics::None, double max_gain = 8.0) const
    {
        check_max_gain(max_gain);
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty() && indices.empty())
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), n, (uint32_t)NCOEFFS, &q));
        std::vector<uint64_t> poff(n + 1), moff(n + 1), ooff(n + 1, 0), soff(sounds.size() + 1, 0);
        std::vector<double> cost(n), samples, out;
        std::vector<uint32_t> len(n), path, map, frames(n);
        int32_t rc = indices.size() == n ? ssym_dtw_align_sizes(resident(), q, indices.data(), nullptr, n, 0, poff.data(),
                                                                moff.data())
                                         : (int32_t)SSYM_E_INVALID;
        if (rc == SSYM_OK) {
            path.resize(2 * poff[n]);
            map.resize(moff[n]);
            rc = ssym_dtw_align(ctx_->get(), resident(), q, indices.data(), nullptr, n, 0, cost.data(), len.data(),
                                poff.data(), path.data(), moff.data(), map.data(), 0);
        }
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        for (std::size_t i = 0; i < sounds.size(); ++i) {
            samples.insert(samples.end(), sounds[i]->samples().begin(), sounds[i]->samples().end());
            soff[i + 1] = samples.size();
        }
        for (uint32_t t = 0; t < n; ++t) {
            ooff[t + 1] = ooff[t] + targets[t]->samples().size();
            frames[t] = (uint32_t)(moff[t + 1] - moff[t]);
        }
        ssym_samples *smp = nullptr;
        ctx_->check(ssym_samples_create(ctx_->get(), samples.data(), soff.data(), (uint32_t)sounds.size(), &smp));
        out.resize(ooff[n]);
        rc = search ? ssym_reconstruct_wsola(ctx_->get(), smp, indices.data(), ooff.data(), n, map.data(), moff.data(),
                                             frames.data(), len.data(), search, 0, nullptr, out.data(), nullptr)
                    : ssym_reconstruct_warped(ctx_->get(), smp, indices.data(), ooff.data(), n, map.data(), moff.data(),
                                              frames.data(), len.data(), 0, out.data(), nullptr);
        ssym_samples_destroy(ctx_->get(), smp);
        ctx_->check(rc);
        return dynamics == Dynamics::Target ? follow_targets(*ctx_, std::move(out), targets, ooff, max_gain) : out;
    }
    // max_gain of the reconstructing methods, refused before any device work whether it is used or not
    static void check_max_gain(double max_gain)
    {
        if (!(max_gain >= 1.0) || max_gain > std::numeric_limits<double>::max())
            throw Error(SSYM_E_INVALID, "max_gain must be finite and at least 1");
    }
    // where inside the dictionary's (unsegmented) recordings every target sounds: subsequence DTW (ssym_spot_queries, or
    // ssym_dtw_spot with indices[t] naming the recording of target t; dtw contexts without a band; the crate has no
    // counterpart).  Frames start_frame ... end_frame (inclusive) of sounds[source_index]; cost is the DTW cost of
    // (those frames, the target), not normalised by any length.  No spot: cost +inf and all three SSYM_NO_MATCH
    struct Spot {
        uint32_t source_index, start_frame, end_frame;
        double cost;
        bool empty() const { return end_frame == SSYM_NO_MATCH; }
    };
    // step: SSYM_STEP_SYMMETRIC (the calls above) or SSYM_STEP_PACED (soundsym_amd.h "Paced spotting": spans of about half
    // to twice the target's frames, and cost / the target's frames a mean per-frame distance)
    std::vector<Spot> spot(const std::vector<ArcSound> &targets, const std::vector<uint32_t> *indices = nullptr,
                           uint32_t step = SSYM_STEP_SYMMETRIC) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty() && (!indices || indices->empty()))
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), n, (uint32_t)NCOEFFS, &q));
        std::vector<uint32_t> idx(n), start(n), end(n);
        std::vector<double> cost(n);
        int32_t rc;
        if (indices) {
            idx = *indices;
            rc = idx.size() != n ? (int32_t)SSYM_E_INVALID
                 : step == SSYM_STEP_SYMMETRIC
                     ? ssym_dtw_spot(ctx_->get(), resident(), q, idx.data(), nullptr, n, 0, cost.data(), start.data(),
                                     end.data(), 0)
                     : ssym_dtw_spot_step(ctx_->get(), resident(), q, idx.data(), nullptr, n, 0, step, cost.data(),
                                          start.data(), end.data(), 0);
        } else {
            rc = step == SSYM_STEP_SYMMETRIC
                     ? ssym_spot_queries(ctx_->get(), resident(), q, 0, idx.data(), cost.data(), start.data(), end.data(), 0)
                     : ssym_spot_queries_step(ctx_->get(), resident(), q, 0, step, idx.data(), cost.data(), start.data(),
                                              end.data(), 0);
        }
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        std::vector<Spot> out(n);
        for (uint32_t t = 0; t < n; ++t)
            out[t] = end[t] == SSYM_NO_MATCH ? Spot{SSYM_NO_MATCH, SSYM_NO_MATCH, SSYM_NO_MATCH, cost[t]}
                                             : Spot{idx[t], start[t], end[t], cost[t]};
        return out;
    }
    // every target tiled by dictionary sounds, cut points and sounds chosen together so that the paced alignment costs of
    // the pieces sum to the least total over every tiling (ssym_dtw_cover; soundsym_amd.h "Cover"; dtw contexts without a
    // band; the crate has no counterpart).  A piece covers frames start_frame ... end_frame (inclusive) of the TARGET with
    // sounds[source_index] at cost, a sum over the piece's frames; total includes piece_penalty per piece.  No cover (no
    // frames, a NaN frame, a stretch no sound can pace): no pieces, total +inf
    struct Cover {
        std::vector<Spot> pieces;
        double total;
        bool empty() const { return pieces.empty(); }
    };
    std::vector<Cover> cover(const std::vector<ArcSound> &targets, double piece_penalty = 0.0) const
    {
        return cover_call(targets, piece_penalty, nullptr);
    }
    // ... with target frames left uncovered at gap_cost per frame (ssym_dtw_cover_gaps; soundsym_amd.h "Cover with gaps";
    // gap_cost >= 0, +inf: no gaps).  A maximal run of gap frames is one entry of pieces with source_index = SSYM_COVER_GAP,
    // its frames start_frame ... end_frame and cost = gap_cost x its frames; total is the call's.  With a finite gap_cost
    // every target with a frame has a cover
    std::vector<Cover> cover(const std::vector<ArcSound> &targets, double piece_penalty, double gap_cost) const
    {
        return cover_call(targets, piece_penalty, &gap_cost);
    }
    // the body of both: gap_cost NULL is ssym_dtw_cover
    std::vector<Cover> cover_call(const std::vector<ArcSound> &targets, double piece_penalty, const double *gap_cost) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty())
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), n, (uint32_t)NCOEFFS, &q));
        const size_t frames = (size_t)(off[n] - off[0]), room = frames ? frames : 1;      // (no NULL of an empty vector)
        std::vector<uint32_t> count(n), src(room), start(room), end(room);
        std::vector<double> total(n), cost(room);
        const int32_t rc = gap_cost ? ssym_dtw_cover_gaps(ctx_->get(), resident(), q, piece_penalty, *gap_cost, 0, count.data(),
                                                          total.data(), src.data(), start.data(), end.data(), cost.data())
                                    : ssym_dtw_cover(ctx_->get(), resident(), q, piece_penalty, 0, count.data(), total.data(),
                                                     src.data(), start.data(), end.data(), cost.data());
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        std::vector<Cover> out(n);
        for (uint32_t t = 0; t < n; ++t) {
            out[t].total = total[t];
            const size_t at = (size_t)(off[t] - off[0]);
            for (uint32_t k = 0; k < count[t]; ++k) {
                std::vector<Spot> &ps = out[t].pieces;
                if (src[at + k] == SSYM_COVER_GAP && !ps.empty() && ps.back().source_index == SSYM_COVER_GAP) {
                    ps.back().end_frame = end[at + k];                       // a run of gap frames is one entry
                    ps.back().cost = *gap_cost * (double)(ps.back().end_frame - ps.back().start_frame + 1);
                } else {
                    ps.push_back(Spot{src[at + k], start[at + k], end[at + k], cost[at + k]});
                }
            }
        }
        return out;
    }
    // every target tiled by free spans of the dictionary's sounds, the cuts, the sounds, the spans and the paced paths chosen
    // together (ssym_dtw_mosaic; soundsym_amd.h "Mosaic"; dtw contexts without a band; the crate has no counterpart): neither
    // side needs cutting beforehand.  A piece plays frames start_frame ... end_frame (inclusive) of the TARGET by frames
    // source_first ... source_last of sounds[source_index] along frame_map (the sound's frame per frame of the piece); cost
    // is the chain of its frame costs (acc = c, acc = c + acc).  gap_cost >= 0 (+inf, the default: no gaps): a maximal run
    // of uncovered frames is one entry with source_index = SSYM_COVER_GAP, source_first = source_last = SSYM_NO_MATCH, no
    // frame_map and cost = the sum of its frames' prices.  total includes piece_penalty per piece and gap_cost per gap
    // frame; frame_costs holds c (or gap_cost) for every target frame.  No mosaic: no pieces, total +inf
    struct MosaicPiece {
        uint32_t source_index, source_first, source_last, start_frame, end_frame;
        double cost;
        std::vector<uint32_t> frame_map;
        bool is_gap() const { return source_index == SSYM_COVER_GAP; }
    };
    struct Mosaic {
        std::vector<MosaicPiece> pieces;
        double total;
        std::vector<double> frame_costs;
        bool empty() const { return pieces.empty(); }
    };
    std::vector<Mosaic> mosaic(const std::vector<ArcSound> &targets, double piece_penalty, double gap_cost = __builtin_inf()) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty())
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), n, (uint32_t)NCOEFFS, &q));
        const size_t frames = (size_t)(off[n] - off[0]), room = frames ? frames : 1;      // (no NULL of an empty vector)
        std::vector<uint32_t> count(n), start(room), src(room), frame(room);
        std::vector<double> total(n), cost(room);
        const int32_t rc = ssym_dtw_mosaic(ctx_->get(), resident(), q, piece_penalty, gap_cost, 0, count.data(), total.data(),
                                           start.data(), src.data(), frame.data(), cost.data());
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        std::vector<Mosaic> out(n);
        for (uint32_t t = 0; t < n; ++t) {
            out[t].total = total[t];
            const size_t at = (size_t)(off[t] - off[0]), T = (size_t)(off[t + 1] - off[t]);
            if (!count[t])
                continue;
            out[t].frame_costs.assign(cost.begin() + at, cost.begin() + at + T);
            std::vector<MosaicPiece> &ps = out[t].pieces;
            for (uint32_t k = 0; k < count[t]; ++k) {
                const size_t s = start[at + k], e = k + 1 < count[t] ? start[at + k + 1] : T;     // frames s ... e - 1
                if (src[at + s] == SSYM_COVER_GAP) {
                    if (!ps.empty() && ps.back().is_gap()) {                 // a run of gap frames is one entry
                        ps.back().end_frame = (uint32_t)s;
                        ps.back().cost = cost[at + s] * (double)(ps.back().end_frame - ps.back().start_frame + 1);
                    } else {
                        ps.push_back(MosaicPiece{SSYM_COVER_GAP, SSYM_NO_MATCH, SSYM_NO_MATCH, (uint32_t)s, (uint32_t)s,
                                                 cost[at + s], {}});
                    }
                    continue;
                }
                double acc = cost[at + s];
                for (size_t j = s + 1; j < e; ++j)
                    acc = cost[at + j] + acc;
                ps.push_back(MosaicPiece{src[at + s], frame[at + s], frame[at + e - 1], (uint32_t)s, (uint32_t)(e - 1), acc,
                                         std::vector<uint32_t>(frame.begin() + at + s, frame.begin() + at + e)});
            }
        }
        return out;
    }
    // align with a Spot per target instead of an index: target t against frames start_frame ... end_frame of
    // sounds[source_index], where they lie in the resident dictionary (ssym_dtw_align_spans; soundsym_amd.h "Span
    // alignment").  path and frame_map count from the span's first frame; an empty Spot gives an empty Alignment
    std::vector<Alignment> align_spans(const std::vector<ArcSound> &targets, const std::vector<Spot> &spots,
                                       uint32_t step = SSYM_STEP_SYMMETRIC) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        if (targets.empty() && spots.empty())
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), n, (uint32_t)NCOEFFS, &q));
        std::vector<uint64_t> poff(n + 1), moff(n + 1);
        std::vector<double> cost(n);
        std::vector<uint32_t> len(n), path, map, src(n), first(n), last(n);
        for (uint32_t t = 0; t < n && t < spots.size(); ++t) {
            src[t] = spots[t].empty() ? SSYM_NO_MATCH : spots[t].source_index;
            first[t] = spots[t].empty() ? SSYM_NO_MATCH : spots[t].start_frame;
            last[t] = spots[t].empty() ? SSYM_NO_MATCH : spots[t].end_frame;
        }
        int32_t rc = spots.size() == n ? ssym_dtw_align_spans_sizes(resident(), q, src.data(), nullptr, first.data(),
                                                                    last.data(), n, 0, poff.data(), moff.data())
                                       : (int32_t)SSYM_E_INVALID;
        if (rc == SSYM_OK) {
            path.resize(2 * poff[n]);
            map.resize(moff[n]);
            rc = ssym_dtw_align_spans(ctx_->get(), resident(), q, src.data(), nullptr, first.data(), last.data(), n, 0, step,
                                      cost.data(), len.data(), poff.data(), path.data(), moff.data(), map.data(), 0);
        }
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        std::vector<Alignment> out(n);
        for (uint32_t t = 0; t < n; ++t) {
            out[t].cost = cost[t];
            out[t].source_index = src[t];
            for (uint32_t s = 0; s < len[t]; ++s)
                out[t].path.push_back({path[2 * (poff[t] + s)], path[2 * (poff[t] + s) + 1]});
            if (len[t])
                out[t].frame_map.assign(map.begin() + moff[t], map.begin() + moff[t + 1]);
        }
        return out;
    }
    // warp with a Spot per target: every span aligned and resynthesised where it lies, the sample window being frame
    // start_frame's first sample up to where frame end_frame + 1 would start, or the recording's end
    // (ssym_dtw_align_spans + ssym_reconstruct_warped_spans, or with search > 0 ssym_reconstruct_wsola_spans).  An empty
    // Spot gives zeros.  dynamics and max_gain as for warp
    std::vector<double> warp_spans(const std::vector<ArcSound> &targets, const std::vector<Spot> &spots, uint32_t search = 0,
                                   uint32_t step = SSYM_STEP_SYMMETRIC, Dynamics dynamics = Dynamics::None,
                                   double max_gain = 8.0) const
    {
        check_max_gain(max_gain);
        const std::vector<Alignment> al = align_spans(targets, spots, step);
        if (targets.empty())
            return {};
        const uint32_t n = (uint32_t)targets.size();
        std::vector<uint64_t> moff(n + 1, 0), ooff(n + 1, 0), soff(sounds.size() + 1, 0), wfirst(n, 0), wlen(n, 0);
        std::vector<uint32_t> map, frames(n), len(n), idx(n, 0);
        std::vector<double> samples, out;
        for (std::size_t i = 0; i < sounds.size(); ++i) {
            samples.insert(samples.end(), sounds[i]->samples().begin(), sounds[i]->samples().end());
            soff[i + 1] = samples.size();
        }
        for (uint32_t t = 0; t < n; ++t) {
            map.insert(map.end(), al[t].frame_map.begin(), al[t].frame_map.end());
            frames[t] = (uint32_t)al[t].frame_map.size();
            len[t] = (uint32_t)al[t].path.size();
            moff[t + 1] = map.size();
            ooff[t + 1] = ooff[t] + targets[t]->samples().size();
            if (spots[t].empty())
                continue;
            idx[t] = spots[t].source_index;
            const uint64_t size = soff[idx[t] + 1] - soff[idx[t]];
            const uint64_t a = std::min<uint64_t>((uint64_t)spots[t].start_frame * SSYM_MFCC_HOP, size);
            const uint64_t b = std::min<uint64_t>(((uint64_t)spots[t].end_frame + 1) * SSYM_MFCC_HOP, size);
            wfirst[t] = a;
            wlen[t] = b > a ? b - a : 0;
        }
        ssym_samples *smp = nullptr;
        ctx_->check(ssym_samples_create(ctx_->get(), samples.data(), soff.data(), (uint32_t)sounds.size(), &smp));
        out.resize(ooff[n]);
        const int32_t rc =
            search ? ssym_reconstruct_wsola_spans(ctx_->get(), smp, idx.data(), wfirst.data(), wlen.data(), ooff.data(), n,
                                                  map.data(), moff.data(), frames.data(), len.data(), search, 0, nullptr,
                                                  out.data(), nullptr)
                   : ssym_reconstruct_warped_spans(ctx_->get(), smp, idx.data(), wfirst.data(), wlen.data(), ooff.data(), n,
                                                   map.data(), moff.data(), frames.data(), len.data(), 0, out.data(), nullptr);
        ssym_samples_destroy(ctx_->get(), smp);
        ctx_->check(rc);
        return dynamics == Dynamics::Target ? follow_targets(*ctx_, std::move(out), targets, ooff, max_gain) : out;
    }
    // every place a target sounds: per target its occurrences by ascending cost, pairwise disjoint within a recording
    // (ssym_dtw_spot_all, one call).  With indices, target t is searched in sounds[indices[t]]; without, in every sound:
    // max_spots (1 ... 64) then applies per sound and a target's list is merged by (cost, source index, end).  max_cost:
    // an occurrence costs at most that (NULL: no threshold).  step as for spot (ssym_dtw_spot_all_step); max_cost stays a sum
    std::vector<std::vector<Spot>> spot_all(const std::vector<ArcSound> &targets, const std::vector<uint32_t> *indices = nullptr,
                                            uint32_t max_spots = 8, const double *max_cost = nullptr,
                                            uint32_t step = SSYM_STEP_SYMMETRIC) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        const uint32_t n = (uint32_t)sounds.size(), m = (uint32_t)targets.size();
        std::vector<std::vector<Spot>> out(m);
        if (m == 0)
            return out;
        std::vector<uint32_t> src, tgt;
        if (indices) {
            src = *indices;
            for (uint32_t t = 0; t < m; ++t)
                tgt.push_back(t);
        } else {
            for (uint32_t s = 0; s < n; ++s)
                for (uint32_t t = 0; t < m; ++t) {
                    src.push_back(s);
                    tgt.push_back(t);
                }
        }
        const size_t np = tgt.size(), K = max_spots;
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), m, (uint32_t)NCOEFFS, &q));
        std::vector<uint32_t> count(np), start(np * K), end(np * K);
        std::vector<double> cost(np * K), limit(max_cost ? np : 0, max_cost ? *max_cost : 0.0);
        const int32_t rc =
            src.size() != np ? (int32_t)SSYM_E_INVALID
            : step == SSYM_STEP_SYMMETRIC
                ? ssym_dtw_spot_all(ctx_->get(), resident(), q, src.data(), tgt.data(), (uint32_t)np, 0, max_spots,
                                    max_cost ? limit.data() : nullptr, count.data(), cost.data(), start.data(), end.data(), 0)
                : ssym_dtw_spot_all_step(ctx_->get(), resident(), q, src.data(), tgt.data(), (uint32_t)np, 0, step, max_spots,
                                         max_cost ? limit.data() : nullptr, count.data(), cost.data(), start.data(),
                                         end.data(), 0);
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        for (size_t p = 0; p < np; ++p)
            for (uint32_t k = 0; k < count[p]; ++k)
                out[tgt[p]].push_back(Spot{src[p], start[p * K + k], end[p * K + k], cost[p * K + k]});
        for (auto &spots : out)
            std::stable_sort(spots.begin(), spots.end(), [](const Spot &a, const Spot &b) {
                if (a.cost != b.cost)
                    return a.cost < b.cost;
                if (a.source_index != b.source_index)
                    return a.source_index < b.source_index;
                return a.end_frame < b.end_frame;
            });
        return out;
    }
    // from_distances' chain of at_distance calls, on the device in one call (ssym_chain)
    std::vector<uint32_t> chain_indices(const Sound &start, const std::vector<double> &distances) const
    {
        if (sounds.empty())
            throw EmptyDictionary();
        std::vector<uint32_t> idx(distances.size());
        ctx_->check(ssym_chain(ctx_->get(), const_cast<ssym_dict *>(resident()), start.mfccs().data(),
                               start.num_frames(), distances.data(), (uint32_t)distances.size(), idx.data(),
                               nullptr));
        return idx;
    }

  private:
    // the dictionary's features are packed once per content change, not per query
    const ssym_dict *resident() const
    {
        // `sounds` is public and mutable (`pub sounds`): entries may have been replaced or reordered in place, so the
        // packed copy is compared by content (the Arcs themselves), not by length; the copy keeps them alive
        if (!dict_ || packed_ != sounds) {
            release();
            std::vector<double> flat;
            std::vector<uint64_t> off;
            pack_features(sounds, flat, off);
            ctx_->check(ssym_dict_create(ctx_->get(), flat.data(), off.data(), (uint32_t)sounds.size(),
                                         (uint32_t)NCOEFFS, &dict_));
            packed_ = sounds;
        }
        return dict_;
    }
    void release() const
    {
        if (dict_)
            ssym_dict_destroy(ctx_->get(), dict_);
        dict_ = nullptr;
    }
    std::shared_ptr<Context> ctx_;
    mutable ssym_dict *dict_ = nullptr;
    mutable std::vector<ArcSound> packed_;
};

// The targets of one query set watched in n_lanes growing sources (ssym_spotter; soundsym_amd.h "Watching"): a push costs
// the new frames alone, best() is SoundDictionary::spot's answer for what a lane has consumed, and occurrences come as
// events under a causal rule (not spot_all's greedy: a span once emitted is never revised).
// step: SSYM_STEP_SYMMETRIC (ssym_spotter_create) or SSYM_STEP_PACED (ssym_spotter_create_step; soundsym_amd.h "Paced
// watching": spans of about half to twice the target's frames, max_cost stays a sum, targets of at most 2048 frames).
class Spotter {
  public:
    using Spot = SoundDictionary::Spot;
    struct Event {
        uint32_t lane, target;
        Spot spot;                  // source_index = the lane
    };
    Spotter(std::shared_ptr<Context> ctx, const std::vector<ArcSound> &targets, uint32_t n_lanes = 1,
            const std::vector<double> *max_cost = nullptr, uint32_t step = SSYM_STEP_SYMMETRIC)
        : ctx_(std::move(ctx)), lanes_(n_lanes), targets_((uint32_t)targets.size())
    {
        if (max_cost && max_cost->size() != targets.size())
            throw Error(SSYM_E_INVALID, "max_cost must hold one value per target");
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), targets_, (uint32_t)NCOEFFS, &q_));
        const double *limits = max_cost ? max_cost->data() : nullptr;
        const int32_t rc = step == SSYM_STEP_SYMMETRIC ? ssym_spotter_create(ctx_->get(), q_, n_lanes, limits, &sp_)
                                                       : ssym_spotter_create_step(ctx_->get(), q_, n_lanes, limits, step, &sp_);
        if (rc != SSYM_OK) {
            ssym_queries_destroy(ctx_->get(), q_);
            ctx_->check(rc);
        }
    }
    ~Spotter()
    {
        ssym_spotter_destroy(ctx_->get(), sp_);      // the spotter reads the queries: it goes first
        ssym_queries_destroy(ctx_->get(), q_);
    }
    Spotter(const Spotter &) = delete;
    Spotter &operator=(const Spotter &) = delete;

    // lane l consumes frames [frame_offsets[l], frame_offsets[l + 1]) of feats (NCOEFFS values each); the events it emits
    std::vector<Event> push(const std::vector<double> &feats, const std::vector<uint64_t> &frame_offsets)
    {
        if (frame_offsets.size() != (size_t)lanes_ + 1)
            throw Error(SSYM_E_INVALID, "frame_offsets must hold n_lanes + 1 entries");
        uint64_t n = 0;
        ctx_->check(ssym_spotter_push(ctx_->get(), sp_, feats.data(), frame_offsets.data(), 0, &n, nullptr, nullptr));
        return events(n);
    }
    // every lane consumes, in place, what the stream's lane holds beyond the frames consumed
    std::vector<Event> follow(const ssym_stream *stream)
    {
        uint64_t n = 0;
        ctx_->check(ssym_spotter_follow(ctx_->get(), sp_, stream, 0, &n, nullptr, nullptr));
        return events(n);
    }
    // "the lane has ended": what it has pending
    std::vector<Event> flush(uint32_t lane)
    {
        uint64_t n = 0;
        ctx_->check(ssym_spotter_flush(ctx_->get(), sp_, lane, &n));
        return events(n);
    }
    // [lane * n_targets + target]: the best span of what the lane has consumed
    std::vector<Spot> best() const
    {
        const size_t np = (size_t)lanes_ * targets_;
        std::vector<double> cost(np);
        std::vector<uint32_t> start(np), end(np);
        ctx_->check(ssym_spotter_best(ctx_->get(), sp_, cost.data(), start.data(), end.data(), 0));
        std::vector<Spot> out(np);
        for (size_t p = 0; p < np; ++p)
            out[p] = end[p] == SSYM_NO_MATCH ? Spot{SSYM_NO_MATCH, SSYM_NO_MATCH, SSYM_NO_MATCH, cost[p]}
                                             : Spot{(uint32_t)(p / targets_), start[p], end[p], cost[p]};
        return out;
    }
    std::vector<uint64_t> counts() const
    {
        std::vector<uint64_t> out(lanes_);
        ctx_->check(ssym_spotter_counts(sp_, out.data()));
        return out;
    }
    void reset(uint32_t lane) { ctx_->check(ssym_spotter_reset(ctx_->get(), sp_, lane)); }

  private:
    std::vector<Event> events(uint64_t n) const
    {
        std::vector<uint32_t> lane(n), tgt(n), start(n), end(n);
        std::vector<double> cost(n);
        if (n)
            ctx_->check(ssym_spotter_events(ctx_->get(), sp_, lane.data(), tgt.data(), cost.data(), start.data(), end.data(), 0));
        std::vector<Event> out(n);
        for (uint64_t k = 0; k < n; ++k)
            out[k] = Event{lane[k], tgt[k], Spot{lane[k], start[k], end[k], cost[k]}};
        return out;
    }
    std::shared_ptr<Context> ctx_;
    uint32_t lanes_ = 0, targets_ = 0;
    ssym_queries *q_ = nullptr;
    ssym_spotter *sp_ = nullptr;
};

// n_lanes growing targets tiled by the segments of a dictionary (ssym_coverer; soundsym_amd.h "Live cover"): every piece is
// reported by the push after which no longer recording could change it, the pieces from reset to flush are
// SoundDictionary::cover's for the whole, and best() gives its total for what a lane has consumed.  The coverer packs the
// sounds' features into a dictionary of its own and keeps it for as long as it lives.
class Coverer {
  public:
    using Spot = SoundDictionary::Spot;
    struct Piece {
        uint32_t lane;
        Spot piece;                 // source_index = the dictionary sound; start / end count the lane's frames, end inclusive
    };
    struct Best {
        double total;               // SoundDictionary::cover's total of everything consumed; +inf without a cover
        uint32_t covered;           // frames of the longest prefix that has a cover
        uint32_t committed;         // frames whose pieces have been emitted
    };
    Coverer(std::shared_ptr<Context> ctx, const std::vector<ArcSound> &sounds, uint32_t n_lanes = 1, double piece_penalty = 0.0)
        : ctx_(std::move(ctx)), lanes_(n_lanes)
    {
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(sounds, flat, off);
        ctx_->check(ssym_dict_create(ctx_->get(), flat.data(), off.data(), (uint32_t)sounds.size(), (uint32_t)NCOEFFS, &dict_));
        const int32_t rc = ssym_coverer_create(ctx_->get(), dict_, n_lanes, piece_penalty, &cv_);
        if (rc != SSYM_OK) {
            ssym_dict_destroy(ctx_->get(), dict_);
            ctx_->check(rc);
        }
    }
    ~Coverer()
    {
        ssym_coverer_destroy(ctx_->get(), cv_);      // the coverer reads the dictionary: it goes first
        ssym_dict_destroy(ctx_->get(), dict_);
    }
    Coverer(const Coverer &) = delete;
    Coverer &operator=(const Coverer &) = delete;

    // lane l consumes frames [frame_offsets[l], frame_offsets[l + 1]) of feats (NCOEFFS values each); the pieces it commits
    std::vector<Piece> push(const std::vector<double> &feats, const std::vector<uint64_t> &frame_offsets)
    {
        if (frame_offsets.size() != (size_t)lanes_ + 1)
            throw Error(SSYM_E_INVALID, "frame_offsets must hold n_lanes + 1 entries");
        uint64_t n = 0;
        ctx_->check(ssym_coverer_push(ctx_->get(), cv_, feats.data(), frame_offsets.data(), 0, &n));
        return pieces(n);
    }
    // every lane consumes, device to device, what the stream's lane holds beyond the frames consumed
    std::vector<Piece> follow(const ssym_stream *stream)
    {
        uint64_t n = 0;
        ctx_->check(ssym_coverer_follow(ctx_->get(), cv_, stream, 0, &n));
        return pieces(n);
    }
    // "the lane has ended": the rest of its cover; the lane consumes nothing more until reset
    std::vector<Piece> flush(uint32_t lane)
    {
        uint64_t n = 0;
        ctx_->check(ssym_coverer_flush(ctx_->get(), cv_, lane, &n));
        return pieces(n);
    }
    std::vector<Best> best() const
    {
        std::vector<double> total(lanes_);
        std::vector<uint32_t> covered(lanes_), committed(lanes_);
        ctx_->check(ssym_coverer_best(ctx_->get(), cv_, total.data(), covered.data(), committed.data(), 0));
        std::vector<Best> out(lanes_);
        for (uint32_t l = 0; l < lanes_; ++l)
            out[l] = Best{total[l], covered[l], committed[l]};
        return out;
    }
    std::vector<uint64_t> counts() const
    {
        std::vector<uint64_t> out(lanes_);
        ctx_->check(ssym_coverer_counts(cv_, out.data(), nullptr));
        return out;
    }
    // frames the ring of back-pointers holds per lane
    uint64_t capacity() const
    {
        uint64_t cap = 0;
        ctx_->check(ssym_coverer_counts(cv_, nullptr, &cap));
        return cap;
    }
    void reset(uint32_t lane) { ctx_->check(ssym_coverer_reset(ctx_->get(), cv_, lane)); }

  private:
    std::vector<Piece> pieces(uint64_t n) const
    {
        std::vector<uint32_t> lane(n), src(n), start(n), end(n);
        std::vector<double> cost(n);
        if (n)
            ctx_->check(ssym_coverer_pieces(ctx_->get(), cv_, lane.data(), src.data(), start.data(), end.data(), cost.data(), 0));
        std::vector<Piece> out(n);
        for (uint64_t k = 0; k < n; ++k)
            out[k] = Piece{lane[k], Spot{src[k], start[k], end[k], cost[k]}};
        return out;
    }
    std::shared_ptr<Context> ctx_;
    uint32_t lanes_ = 0;
    ssym_dict *dict_ = nullptr;
    ssym_coverer *cv_ = nullptr;
};

// n_lanes growing targets tiled by free spans of a dictionary's uncut recordings (ssym_mosaicker; soundsym_amd.h "Live
// mosaic"): every target frame is reported by the push after which no longer recording could change it, the frames from
// reset to flush are SoundDictionary::mosaic's for the whole, and best() gives its total for what a lane has consumed.  The
// mosaicker packs the sounds' features into a dictionary of its own and keeps it for as long as it lives.
class Mosaicker {
  public:
    struct Frame {
        uint32_t lane;
        uint32_t column;            // the lane's frame, counted since its reset
        uint32_t src;               // the dictionary sound, or SSYM_COVER_GAP
        uint32_t frame;             // the sound's frame (SSYM_NO_MATCH on a gap frame)
        double cost;                // c of the pair, or gap_cost
        bool start;                 // a piece or a gap frame starts here
    };
    struct Best {
        double total;               // SoundDictionary::mosaic's total of everything consumed; +inf without a mosaic
        uint32_t covered;           // frames of the longest prefix that has a mosaic
        uint32_t committed;         // frames that have been emitted
    };
    // gap_cost +inf: no gaps
    Mosaicker(std::shared_ptr<Context> ctx, const std::vector<ArcSound> &sounds, uint32_t n_lanes = 1, double piece_penalty = 0.0,
              double gap_cost = std::numeric_limits<double>::infinity())
        : ctx_(std::move(ctx)), lanes_(n_lanes)
    {
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(sounds, flat, off);
        ctx_->check(ssym_dict_create(ctx_->get(), flat.data(), off.data(), (uint32_t)sounds.size(), (uint32_t)NCOEFFS, &dict_));
        const int32_t rc = ssym_mosaicker_create(ctx_->get(), dict_, n_lanes, piece_penalty, gap_cost, &mk_);
        if (rc != SSYM_OK) {
            ssym_dict_destroy(ctx_->get(), dict_);
            ctx_->check(rc);
        }
    }
    ~Mosaicker()
    {
        ssym_mosaicker_destroy(ctx_->get(), mk_);    // the mosaicker reads the dictionary: it goes first
        ssym_dict_destroy(ctx_->get(), dict_);
    }
    Mosaicker(const Mosaicker &) = delete;
    Mosaicker &operator=(const Mosaicker &) = delete;

    // lane l consumes frames [frame_offsets[l], frame_offsets[l + 1]) of feats (NCOEFFS values each); the frames it commits
    std::vector<Frame> push(const std::vector<double> &feats, const std::vector<uint64_t> &frame_offsets)
    {
        if (frame_offsets.size() != (size_t)lanes_ + 1)
            throw Error(SSYM_E_INVALID, "frame_offsets must hold n_lanes + 1 entries");
        uint64_t n = 0;
        ctx_->check(ssym_mosaicker_push(ctx_->get(), mk_, feats.data(), frame_offsets.data(), 0, &n));
        return frames(n);
    }
    // every lane consumes, device to device, what the stream's lane holds beyond the frames consumed
    std::vector<Frame> follow(const ssym_stream *stream)
    {
        uint64_t n = 0;
        ctx_->check(ssym_mosaicker_follow(ctx_->get(), mk_, stream, 0, &n));
        return frames(n);
    }
    // "the lane has ended": the rest of its mosaic; the lane consumes nothing more until reset
    std::vector<Frame> flush(uint32_t lane)
    {
        uint64_t n = 0;
        ctx_->check(ssym_mosaicker_flush(ctx_->get(), mk_, lane, &n));
        return frames(n);
    }
    std::vector<Best> best() const
    {
        std::vector<double> total(lanes_);
        std::vector<uint32_t> covered(lanes_), committed(lanes_);
        ctx_->check(ssym_mosaicker_best(ctx_->get(), mk_, total.data(), covered.data(), committed.data(), 0));
        std::vector<Best> out(lanes_);
        for (uint32_t l = 0; l < lanes_; ++l)
            out[l] = Best{total[l], covered[l], committed[l]};
        return out;
    }
    std::vector<uint64_t> counts() const
    {
        std::vector<uint64_t> out(lanes_);
        ctx_->check(ssym_mosaicker_counts(mk_, out.data(), nullptr));
        return out;
    }
    // columns the ring of uncommitted columns holds per lane
    uint64_t capacity() const
    {
        uint64_t cap = 0;
        ctx_->check(ssym_mosaicker_counts(mk_, nullptr, &cap));
        return cap;
    }
    void reset(uint32_t lane) { ctx_->check(ssym_mosaicker_reset(ctx_->get(), mk_, lane)); }
    // the library's handle: what Resynth::take reads the last frame log from
    const ssym_mosaicker *handle() const { return mk_; }

  private:
    std::vector<Frame> frames(uint64_t n) const
    {
        std::vector<uint32_t> lane(n), column(n), src(n), frame(n), start(n);
        std::vector<double> cost(n);
        if (n)
            ctx_->check(ssym_mosaicker_frames(ctx_->get(), mk_, lane.data(), column.data(), src.data(), frame.data(), cost.data(),
                                              start.data(), 0));
        std::vector<Frame> out(n);
        for (uint64_t k = 0; k < n; ++k)
            out[k] = Frame{lane[k], column[k], src[k], frame[k], cost[k], start[k] != 0};
        return out;
    }
    std::shared_ptr<Context> ctx_;
    uint32_t lanes_ = 0;
    ssym_dict *dict_ = nullptr;
    ssym_mosaicker *mk_ = nullptr;
};

// n_lanes lanes of live resynthesis from a dictionary's samples (ssym_resynth; soundsym_amd.h "Live resynthesis"): a lane
// takes committed mosaic frames -- a Mosaicker's last frame log device to device (take) or host rows (push) -- and every call
// returns the samples it releases, those whose bits no later frame can change; from reset to flush a lane's samples are the
// offline piece-by-piece resynthesis of the finished mosaic, bit for bit.  The resynthesiser makes the sounds' samples
// resident in a store of its own and keeps it for as long as it lives.
class Resynth {
  public:
    struct Frame {
        uint32_t lane;
        uint32_t column;            // the lane's frame, counted since its reset
        uint32_t src;               // the dictionary sound, or SSYM_COVER_GAP
        uint32_t frame;             // the sound's frame
        bool start;                 // a piece or a gap frame starts here
    };
    struct Samples {
        std::vector<uint64_t> lane_offsets;     // n_lanes + 1: lane l's samples are [lane_offsets[l], lane_offsets[l + 1])
        std::vector<double> samples;
        std::vector<int32_t> pcm32;
    };
    // search: WSOLA's width in samples, at most 512; 0 is the plain warp
    Resynth(std::shared_ptr<Context> ctx, const std::vector<ArcSound> &sounds, uint32_t n_lanes = 1, uint32_t search = 0)
        : ctx_(std::move(ctx)), lanes_(n_lanes)
    {
        std::vector<double> samples;
        std::vector<uint64_t> soff(sounds.size() + 1, 0);
        for (std::size_t i = 0; i < sounds.size(); ++i) {
            samples.insert(samples.end(), sounds[i]->samples().begin(), sounds[i]->samples().end());
            soff[i + 1] = samples.size();
        }
        ctx_->check(ssym_samples_create(ctx_->get(), samples.data(), soff.data(), (uint32_t)sounds.size(), &store_));
        const int32_t rc = ssym_resynth_create(ctx_->get(), store_, n_lanes, search, &rs_);
        if (rc != SSYM_OK) {
            ssym_samples_destroy(ctx_->get(), store_);
            ctx_->check(rc);
        }
    }
    ~Resynth()
    {
        ssym_resynth_destroy(ctx_->get(), rs_);      // the resynthesiser reads the store: it goes first
        ssym_samples_destroy(ctx_->get(), store_);
    }
    Resynth(const Resynth &) = delete;
    Resynth &operator=(const Resynth &) = delete;

    // frames ordered by (lane, column) -- a Mosaicker's frames pass straight in; the samples they release
    Samples push(const std::vector<Frame> &frames)
    {
        const size_t n = frames.size();
        std::vector<uint32_t> lane(n), column(n), src(n), frame(n), start(n);
        for (size_t k = 0; k < n; ++k) {
            lane[k] = frames[k].lane, column[k] = frames[k].column, src[k] = frames[k].src, frame[k] = frames[k].frame;
            start[k] = frames[k].start ? 1u : 0u;
        }
        uint64_t got = 0;
        ctx_->check(ssym_resynth_push(ctx_->get(), rs_, lane.data(), column.data(), src.data(), frame.data(), start.data(), n, &got));
        return samples(got);
    }
    Samples push(const std::vector<Mosaicker::Frame> &frames)
    {
        std::vector<Frame> rows(frames.size());
        for (size_t k = 0; k < frames.size(); ++k)
            rows[k] = Frame{frames[k].lane, frames[k].column, frames[k].src, frames[k].frame, frames[k].start};
        return push(rows);
    }
    // the mosaicker's last frame log, consumed where it lies: no frame goes through the host
    Samples take(const Mosaicker &mk)
    {
        uint64_t got = 0;
        ctx_->check(ssym_resynth_take(ctx_->get(), rs_, mk.handle(), &got));
        return samples(got);
    }
    // "the lane has ended with total_samples samples": the rest, the tail behind the last frame included
    Samples flush(uint32_t lane, uint64_t total_samples)
    {
        uint64_t got = 0;
        ctx_->check(ssym_resynth_flush(ctx_->get(), rs_, lane, total_samples, &got));
        return samples(got);
    }
    // frames consumed per lane since its reset
    std::vector<uint64_t> counts() const
    {
        std::vector<uint64_t> out(lanes_);
        ctx_->check(ssym_resynth_counts(rs_, out.data(), nullptr));
        return out;
    }
    // samples released per lane since its reset
    std::vector<uint64_t> released() const
    {
        std::vector<uint64_t> out(lanes_);
        ctx_->check(ssym_resynth_counts(rs_, nullptr, out.data()));
        return out;
    }
    void reset(uint32_t lane) { ctx_->check(ssym_resynth_reset(ctx_->get(), rs_, lane)); }

  private:
    Samples samples(uint64_t n) const
    {
        Samples out{std::vector<uint64_t>((size_t)lanes_ + 1, 0), std::vector<double>(n), std::vector<int32_t>(n)};
        ctx_->check(ssym_resynth_samples(ctx_->get(), rs_, out.lane_offsets.data(), n ? out.samples.data() : nullptr,
                                         n ? out.pcm32.data() : nullptr, 0));
        return out;
    }
    std::shared_ptr<Context> ctx_;
    uint32_t lanes_ = 0;
    ssym_samples *store_ = nullptr;
    ssym_resynth *rs_ = nullptr;
};

// Live envelope following (ssym_follower_*, "Live envelope following" in soundsym_amd.h): follow_envelope's resumable form.
// A lane takes the resynthesis and the reference -- the target's own samples -- as they grow, in any amounts, and every
// push returns what it releases: the hops whose two gain boundaries are settled, two hops of look-ahead on both signals.
// From reset to flush a lane's samples and gains are follow_envelope's for what it consumed, bit for bit.
class Follower {
  public:
    struct Samples {
        std::vector<uint64_t> lane_offsets;     // n_lanes + 1: lane l's samples are [lane_offsets[l], lane_offsets[l + 1])
        std::vector<double> samples;
        std::vector<int32_t> pcm32;
        std::vector<uint64_t> gain_offsets;     // n_lanes + 1: the gains of the boundaries the call settled, lane by lane
        std::vector<double> gains;
    };
    struct Counts {
        std::vector<uint64_t> ny, nx, released; // per lane since its reset: consumed of either signal, samples released
    };
    // max_gain: finite and at least 1; n_lanes 1 ... 16384
    explicit Follower(std::shared_ptr<Context> ctx, uint32_t n_lanes = 1, double max_gain = 8.0) : ctx_(std::move(ctx)), lanes_(n_lanes)
    {
        ctx_->check(ssym_follower_create(ctx_->get(), n_lanes, max_gain, &fl_));
    }
    ~Follower() { ssym_follower_destroy(ctx_->get(), fl_); }
    Follower(const Follower &) = delete;
    Follower &operator=(const Follower &) = delete;

    // lane l consumes samples[sample_offsets[l] ... sample_offsets[l + 1]) and ref[ref_offsets[l] ... ref_offsets[l + 1])
    Samples push(const std::vector<double> &samples, const std::vector<uint64_t> &sample_offsets, const std::vector<double> &ref,
                 const std::vector<uint64_t> &ref_offsets)
    {
        if (sample_offsets.size() != (size_t)lanes_ + 1 || ref_offsets.size() != (size_t)lanes_ + 1)
            throw Error(SSYM_E_INVALID, "Follower::push: n_lanes + 1 sample_offsets and n_lanes + 1 ref_offsets");
        if (samples.size() < sample_offsets.back() || ref.size() < ref_offsets.back())
            throw Error(SSYM_E_INVALID, "Follower::push: samples or ref hold fewer values than their offsets ask for");
        uint64_t got = 0;
        ctx_->check(ssym_follower_push(ctx_->get(), fl_, samples.empty() ? nullptr : samples.data(), sample_offsets.data(),
                                       ref.empty() ? nullptr : ref.data(), ref_offsets.data(), 0, &got));
        return samples_of_last_call();
    }
    // a follower of one lane takes the bare signals
    Samples push(const std::vector<double> &samples, const std::vector<double> &ref)
    {
        return push(samples, {0, samples.size()}, ref, {0, ref.size()});
    }
    // "the lane has ended": the remaining boundaries with the offline clipping, the rest of the resynthesis
    Samples flush(uint32_t lane = 0)
    {
        uint64_t got = 0;
        ctx_->check(ssym_follower_flush(ctx_->get(), fl_, lane, &got));
        return samples_of_last_call();
    }
    Counts counts() const
    {
        Counts c{std::vector<uint64_t>(lanes_), std::vector<uint64_t>(lanes_), std::vector<uint64_t>(lanes_)};
        ctx_->check(ssym_follower_counts(fl_, c.ny.data(), c.nx.data(), c.released.data()));
        return c;
    }
    void reset(uint32_t lane = 0) { ctx_->check(ssym_follower_reset(ctx_->get(), fl_, lane)); }

  private:
    Samples samples_of_last_call() const
    {
        Samples out;
        out.lane_offsets.assign((size_t)lanes_ + 1, 0);
        out.gain_offsets.assign((size_t)lanes_ + 1, 0);
        ctx_->check(ssym_follower_samples(ctx_->get(), fl_, out.lane_offsets.data(), nullptr, nullptr, out.gain_offsets.data(), nullptr, 0));
        out.samples.resize(out.lane_offsets.back());
        out.pcm32.resize(out.lane_offsets.back());
        out.gains.resize(out.gain_offsets.back());
        ctx_->check(ssym_follower_samples(ctx_->get(), fl_, nullptr, out.samples.empty() ? nullptr : out.samples.data(),
                                          out.pcm32.empty() ? nullptr : out.pcm32.data(), nullptr,
                                          out.gains.empty() ? nullptr : out.gains.data(), 0));
        return out;
    }
    std::shared_ptr<Context> ctx_;
    uint32_t lanes_ = 0;
    ssym_follower *fl_ = nullptr;
};

// One rank of a SoundDictionary split over the GPUs of one node (source-axis shards, one rank -- thread or process --
// per GPU): rank g holds sounds [lo, lo + shard.size()) of the whole dictionary and is handed the same targets as every
// other rank; match_indices returns GLOBAL indices, the same complete answer on every rank, bit for bit the unsharded
// one.  The collectives (RCCL all-reduce(MIN) of the per-target bounds, all-gather of (cost, index)) run inside the
// library on the context's stream (ssym_match_sharded): the loop of clone_from_dictionary / morph_to,
// src/sound.rs:451-455 / 440-446, for a dictionary too large or too slow for one GPU.
class ShardedDictionary {
  public:
    using Id = std::vector<unsigned char>;
    // rank 0 draws the id (ncclGetUniqueId) and hands it to the other ranks by whatever means the host has
    static Id unique_id()
    {
        Id id(SSYM_COMM_ID_BYTES);
        int rc = ssym_comm_unique_id(id.data());
        if (rc != SSYM_OK)
            throw Error(rc, "ssym_comm_unique_id failed (is RCCL available?)");
        return id;
    }
    // collective over all `world` ranks (ncclCommInitRank)
    ShardedDictionary(std::shared_ptr<Context> ctx, const Id &id, int rank, int world, std::vector<ArcSound> shard,
                      uint32_t lo)
        : ctx_(std::move(ctx)), shard_(std::move(shard)), lo_(lo)
    {
        ctx_->check(ssym_comm_create(ctx_->get(), id.data(), rank, world, &comm_));
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(shard_, flat, off);
        int rc = ssym_dict_create(ctx_->get(), flat.data(), off.data(), (uint32_t)shard_.size(), (uint32_t)NCOEFFS, &dict_);
        if (rc != SSYM_OK) {
            ssym_comm_destroy(ctx_->get(), comm_);
            ctx_->check(rc);
        }
    }
    ~ShardedDictionary()
    {
        ssym_dict_destroy(ctx_->get(), dict_);
        ssym_comm_destroy(ctx_->get(), comm_);
    }
    ShardedDictionary(const ShardedDictionary &) = delete;
    ShardedDictionary &operator=(const ShardedDictionary &) = delete;

    std::vector<uint32_t> match_indices(const std::vector<ArcSound> &targets, const double *distances) const
    {
        std::vector<double> flat;
        std::vector<uint64_t> off;
        pack_features(targets, flat, off);
        ssym_queries *q = nullptr;
        ctx_->check(ssym_queries_create(ctx_->get(), flat.data(), off.data(), (uint32_t)targets.size(),
                                        (uint32_t)NCOEFFS, &q));
        std::vector<uint32_t> idx(targets.size());
        int32_t rc = ssym_match_sharded(ctx_->get(), comm_, dict_, q, distances, lo_, idx.data(), nullptr, 0);
        ssym_queries_destroy(ctx_->get(), q);
        ctx_->check(rc);
        return idx;
    }

  private:
    std::shared_ptr<Context> ctx_;
    std::vector<ArcSound> shard_;
    uint32_t lo_;
    ssym_comm *comm_ = nullptr;
    ssym_dict *dict_ = nullptr;
};

class SoundSequence {
  public:
    static SoundSequence new_(std::vector<ArcSound> sounds)   // :392
    {
        SoundSequence s;
        s.sounds_ = std::move(sounds);
        return s;
    }
    const std::vector<ArcSound> &sounds() const { return sounds_; }   // :432

    // :405-417 greedy chain: each step's query is the previous result; the steps run on the device
    // back to back (one call, one wait)
    static SoundSequence from_distances(const std::vector<double> &distances, ArcSound start,
                                        const SoundDictionary &dict)
    {
        std::vector<ArcSound> sounds{start};
        if (!distances.empty())
            for (uint32_t i : dict.chain_indices(*start, distances))
                sounds.push_back(dict.sounds[i]);
        return new_(std::move(sounds));
    }
    // :440-449 zip(sounds, distances) -> at_distance, as ONE batch
    SoundSequence morph_to(const std::vector<double> &distances, const SoundDictionary &dict) const
    {
        std::size_t n = std::min(sounds_.size(), distances.size());
        std::vector<ArcSound> q(sounds_.begin(), sounds_.begin() + n), out;
        if (n == 0)
            return new_({});
        for (uint32_t i : dict.match_indices(q, distances.data()))
            out.push_back(dict.sounds[i]);
        return new_(std::move(out));
    }
    // :451-472 match every sound, then fit the match to the target's length (:456-465)
    SoundSequence clone_from_dictionary(const SoundDictionary &dict) const
    {
        if (sounds_.empty())
            return new_({});
        std::vector<ArcSound> out;
        auto idx = dict.match_indices(sounds_, nullptr);
        for (std::size_t k = 0; k < sounds_.size(); ++k) {
            const ArcSound &sound = sounds_[k], &s = dict.sounds[idx[k]];
            if (sound->samples().size() == s->samples().size()) {
                out.push_back(s);   // :463-464 shares the Arc
            } else {
                std::vector<double> samps(sound->samples().size(), 0.0);   // :457-462
                std::copy_n(s->samples().begin(), std::min(samps.size(), s->samples().size()), samps.begin());
                out.push_back(std::make_shared<const Sound>(
                    Sound::from_samples(std::move(samps), sound->sample_rate(), std::nullopt, std::nullopt)));
            }
        }
        return new_(std::move(out));
    }
    Sound to_sound() const   // :475-483
    {
        std::vector<double> samples;
        for (const auto &s : sounds_)
            samples.insert(samples.end(), s->samples().begin(), s->samples().end());
        double rate = sounds_.empty() ? 44100.0 : sounds_[0]->sample_rate();
        return Sound::from_samples(std::move(samples), rate, std::nullopt, std::nullopt);
    }

  private:
    std::vector<ArcSound> sounds_;
};

}  // namespace soundsym
