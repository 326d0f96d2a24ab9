// tests/cpp/test_mirror_dtw.cpp -- every DTW-family method of the C++ mirror (include/soundsym.hpp) run once on the case
// set of tests/mirror_cases.py, the results written out for tests/test_gpu_mirror_dtw.py to compare, call for call, with
// the Python mirror's on the same sounds.
//
//   test_mirror_dtw <case file> <result file>
//
// Both files are the container of tests/mirror_cases.py (named little-endian arrays of f64, u32 or u64).  The program
// asserts nothing about values.  Every call runs inside run(name, ...), which records "<name>.code": 0 when the call
// returned, the exception's code when it threw a soundsym::Error.  Exit code 0 = every call did one of the two.
//
// Build: tests/cpp/Makefile.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>

#include "soundsym.hpp"

using namespace soundsym;
using Spot = SoundDictionary::Spot;
using Alignment = SoundDictionary::Alignment;
using Sounds = std::vector<ArcSound>;

// ---- the container -------------------------------------------------------------------------------------------------
struct Array {
    uint8_t dtype = 0;                  // 0 f64, 1 u32, 2 u64
    std::vector<double> f;
    std::vector<uint32_t> u;
    std::vector<uint64_t> w;
};
static const char MAGIC[9] = "SSYMARR1";
static std::map<std::string, Array> g_in;
static std::vector<std::pair<std::string, Array>> g_out;
static int g_bad = 0;

template <class T>
static bool take(const std::string &buf, size_t &at, uint64_t count, std::vector<T> &out)
{
    if (count > (buf.size() - at) / sizeof(T))
        return false;
    out.resize(count);
    if (count)
        std::memcpy(out.data(), buf.data() + at, count * sizeof(T));
    at += count * sizeof(T);
    return true;
}

static bool read_arrays(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    std::string buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (!f || buf.size() < 12 || std::memcmp(buf.data(), MAGIC, 8) != 0)
        return false;
    uint32_t n;
    std::memcpy(&n, buf.data() + 8, 4);
    size_t at = 12;
    for (uint32_t k = 0; k < n; ++k) {
        if (at >= buf.size())
            return false;
        const size_t len = (uint8_t)buf[at];
        if (len == 0 || at + 1 + len + 9 > buf.size())
            return false;
        const std::string name = buf.substr(at + 1, len);
        Array a;
        a.dtype = (uint8_t)buf[at + 1 + len];
        uint64_t count;
        std::memcpy(&count, buf.data() + at + 2 + len, 8);
        at += 1 + len + 9;
        const bool ok = a.dtype == 0 ? take(buf, at, count, a.f) : a.dtype == 1 ? take(buf, at, count, a.u)
                        : a.dtype == 2 ? take(buf, at, count, a.w) : false;
        if (!ok)
            return false;
        g_in[name] = std::move(a);
    }
    return at == buf.size();
}

static bool write_arrays(const char *path)
{
    std::ofstream f(path, std::ios::binary);
    const uint32_t n = (uint32_t)g_out.size();
    f.write(MAGIC, 8);
    f.write((const char *)&n, 4);
    for (const auto &e : g_out) {
        const Array &a = e.second;
        const uint8_t len = (uint8_t)e.first.size();
        const uint64_t count = a.dtype == 0 ? a.f.size() : a.dtype == 1 ? a.u.size() : a.w.size();
        f.write((const char *)&len, 1);
        f.write(e.first.data(), len);
        f.write((const char *)&a.dtype, 1);
        f.write((const char *)&count, 8);
        if (a.dtype == 0)
            f.write((const char *)a.f.data(), (std::streamsize)(count * 8));
        else if (a.dtype == 1)
            f.write((const char *)a.u.data(), (std::streamsize)(count * 4));
        else
            f.write((const char *)a.w.data(), (std::streamsize)(count * 8));
    }
    f.flush();
    return (bool)f;
}

static void put(const std::string &name, std::vector<double> v)
{
    Array a;
    a.dtype = 0;
    a.f = std::move(v);
    g_out.emplace_back(name, std::move(a));
}
static void put(const std::string &name, std::vector<uint32_t> v)
{
    Array a;
    a.dtype = 1;
    a.u = std::move(v);
    g_out.emplace_back(name, std::move(a));
}
static void put(const std::string &name, std::vector<uint64_t> v)
{
    Array a;
    a.dtype = 2;
    a.w = std::move(v);
    g_out.emplace_back(name, std::move(a));
}

static const Array &in(const std::string &name)
{
    auto it = g_in.find(name);
    if (it == g_in.end())
        throw std::runtime_error("the case file has no array " + name);
    return it->second;
}

// ---- results as arrays ---------------------------------------------------------------------------------------------
static void put_alignments(const std::string &p, const std::vector<Alignment> &al)
{
    std::vector<double> cost;
    std::vector<uint32_t> src, path, map;
    std::vector<uint64_t> poff{0}, moff{0};
    for (const auto &a : al) {
        cost.push_back(a.cost);
        src.push_back(a.source_index);
        for (const auto &cell : a.path) {
            path.push_back(cell[0]);
            path.push_back(cell[1]);
        }
        map.insert(map.end(), a.frame_map.begin(), a.frame_map.end());
        poff.push_back(path.size() / 2);
        moff.push_back(map.size());
    }
    put(p + ".cost", cost);
    put(p + ".src", src);
    put(p + ".path_off", poff);
    put(p + ".path", path);
    put(p + ".map_off", moff);
    put(p + ".map", map);
}

static void put_spots(const std::string &p, const std::vector<Spot> &spots)
{
    std::vector<double> cost;
    std::vector<uint32_t> src, start, end;
    for (const auto &s : spots) {
        cost.push_back(s.cost);
        src.push_back(s.source_index);
        start.push_back(s.start_frame);
        end.push_back(s.end_frame);
    }
    put(p + ".cost", cost);
    put(p + ".src", src);
    put(p + ".start", start);
    put(p + ".end", end);
}

static void put_spot_lists(const std::string &p, const std::vector<std::vector<Spot>> &lists)
{
    std::vector<uint64_t> off{0};
    std::vector<Spot> flat;
    for (const auto &l : lists) {
        flat.insert(flat.end(), l.begin(), l.end());
        off.push_back(flat.size());
    }
    put(p + ".off", off);
    put_spots(p, flat);
}

static void put_events(const std::string &p, const std::vector<Spotter::Event> &events)
{
    std::vector<uint32_t> lane, target;
    std::vector<Spot> spots;
    for (const auto &e : events) {
        lane.push_back(e.lane);
        target.push_back(e.target);
        spots.push_back(e.spot);
    }
    put(p + ".lane", lane);
    put(p + ".target", target);
    put_spots(p, spots);
}

// a list of lists of the dictionary's own sounds as indices into it (SSYM_NO_MATCH: a sound that is none of them)
static void put_sound_lists(const std::string &p, const std::vector<Sounds> &lists, const SoundDictionary &d)
{
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> idx;
    for (const auto &l : lists) {
        for (const auto &s : l) {
            const auto it = std::find(d.sounds.begin(), d.sounds.end(), s);
            idx.push_back(it == d.sounds.end() ? SSYM_NO_MATCH : (uint32_t)(it - d.sounds.begin()));
        }
        off.push_back(idx.size());
    }
    put(p + ".off", off);
    put(p + ".idx", idx);
}

static void run(const std::string &name, const std::function<void()> &call)
{
    double code = 0.0;
    try {
        call();
    } catch (const Error &e) {
        code = (double)e.code;
    } catch (const std::exception &e) {
        std::printf("%s: %s\n", name.c_str(), e.what());
        code = 9999.0;
        ++g_bad;
    }
    put(name + ".code", std::vector<double>{code});
}

// ---- the cases -----------------------------------------------------------------------------------------------------
static Sounds sounds_of(const std::string &kind)
{
    Sounds out;
    for (int i = 0;; ++i) {
        const std::string base = kind + std::to_string(i);
        if (!g_in.count(base + ".mfccs"))
            return out;
        out.push_back(std::make_shared<const Sound>(
            Sound::from_samples(in(base + ".samples").f, 44100.0, in(base + ".mfccs").f, std::nullopt)));
    }
}

static const char *step_name(uint32_t step) { return step == SSYM_STEP_PACED ? "paced" : "sym"; }
static const uint32_t STEPS[2] = {SSYM_STEP_SYMMETRIC, SSYM_STEP_PACED};

static Spot no_spot()
{
    return Spot{SSYM_NO_MATCH, SSYM_NO_MATCH, SSYM_NO_MATCH, std::numeric_limits<double>::infinity()};
}

static std::vector<Spot> heads(const std::vector<std::vector<Spot>> &lists)
{
    std::vector<Spot> out;
    for (const auto &l : lists)
        out.push_back(l.empty() ? no_spot() : l[0]);
    return out;
}

// the frames [first, first + count) of a recording, appended to feats
static void append_frames(std::vector<double> &feats, const Sound &rec, uint64_t first, uint64_t count)
{
    const auto &m = rec.mfccs();
    feats.insert(feats.end(), m.begin() + (std::ptrdiff_t)(first * NCOEFFS), m.begin() + (std::ptrdiff_t)((first + count) * NCOEFFS));
}

// one Spotter case: the lanes' recordings pushed block by block, every lane flushed, one lane reset and fed again
static void spotter_case(const std::string &p, const std::shared_ptr<Context> &ctx, const Sounds &tgts, const Sounds &recs,
                         const std::vector<uint32_t> &lane_rec, const std::vector<uint64_t> &pushes, uint32_t again,
                         const std::vector<double> *max_cost, uint32_t step)
{
    const uint32_t lanes = (uint32_t)lane_rec.size();
    const size_t n_push = pushes.size() / lanes;
    Spotter sp(ctx, tgts, lanes, max_cost, step);
    std::vector<uint64_t> done(lanes, 0);
    for (size_t k = 0; k < n_push; ++k) {
        std::vector<double> feats;
        std::vector<uint64_t> off{0};
        for (uint32_t l = 0; l < lanes; ++l) {
            append_frames(feats, *recs[lane_rec[l]], done[l], pushes[k * lanes + l]);
            done[l] += pushes[k * lanes + l];
            off.push_back(feats.size() / NCOEFFS);
        }
        const std::string q = p + ".push" + std::to_string(k);
        put_events(q, sp.push(feats, off));
        put_spots(q + ".best", sp.best());
        put(q + ".counts", sp.counts());
    }
    for (uint32_t l = 0; l < lanes; ++l)
        put_events(p + ".flush" + std::to_string(l), sp.flush(l));
    sp.reset(again);
    put(p + ".reset.counts", sp.counts());
    put_spots(p + ".reset.best", sp.best());
    uint64_t at = 0;
    for (size_t k = 0; k < n_push; ++k) {
        std::vector<double> feats;
        std::vector<uint64_t> off{0};
        for (uint32_t l = 0; l < lanes; ++l) {
            if (l == again)
                append_frames(feats, *recs[lane_rec[l]], at, pushes[k * lanes + l]);
            off.push_back(feats.size() / NCOEFFS);
        }
        at += pushes[k * lanes + again];
        put_events(p + ".again" + std::to_string(k), sp.push(feats, off));
    }
    put_events(p + ".again.flush", sp.flush(again));
    put_spots(p + ".again.best", sp.best());
    put(p + ".again.counts", sp.counts());
}

// every method of the family once, for the refusals that do not depend on the arguments (a refcos context, an empty
// dictionary) and for the empty target list
static void every_method(const std::string &p, const std::shared_ptr<Context> &ctx, SoundDictionary &d, const Sounds &tgts,
                         bool with_spotter)
{
    const uint32_t n = (uint32_t)tgts.size();
    const std::vector<uint32_t> idx(n, 0);
    const std::vector<Spot> spots(n, Spot{0, 0, 0, 0.0});
    run(p + ".match_indices_step", [&] {
        std::vector<double> costs{1.0};
        put(p + ".match_indices_step.idx", d.match_indices_step(tgts, nullptr, SSYM_STEP_PACED, &costs));
        put(p + ".match_indices_step.cost", costs);
    });
    run(p + ".pair_matrix_step", [&] { put(p + ".pair_matrix_step.out", d.pair_matrix_step(tgts, SSYM_STEP_PACED)); });
    run(p + ".candidates", [&] { put_sound_lists(p + ".candidates", d.candidates(tgts, 2), d); });
    for (uint32_t step : STEPS) {
        const std::string s = std::string(".") + step_name(step);
        run(p + ".align" + s, [&] { put_alignments(p + ".align" + s, d.align(tgts, idx, step)); });
        run(p + ".spot" + s, [&] { put_spots(p + ".spot" + s, d.spot(tgts, nullptr, step)); });
        run(p + ".spot.idx" + s, [&] { put_spots(p + ".spot.idx" + s, d.spot(tgts, &idx, step)); });
        run(p + ".spot_all" + s, [&] { put_spot_lists(p + ".spot_all" + s, d.spot_all(tgts, nullptr, 8, nullptr, step)); });
        run(p + ".spot_all.idx" + s, [&] { put_spot_lists(p + ".spot_all.idx" + s, d.spot_all(tgts, &idx, 8, nullptr, step)); });
        run(p + ".align_spans" + s, [&] { put_alignments(p + ".align_spans" + s, d.align_spans(tgts, spots, step)); });
        run(p + ".warp_spans" + s, [&] { put(p + ".warp_spans" + s, d.warp_spans(tgts, spots, 0, step)); });
        if (with_spotter)
            run(p + ".spotter" + s, [&] {
                Spotter sp(ctx, tgts, 2, nullptr, step);
                put(p + ".spotter" + s + ".counts", sp.counts());
                put_spots(p + ".spotter" + s + ".best", sp.best());
            });
    }
    run(p + ".warp", [&] { put(p + ".warp.out", d.warp(tgts, idx, 0)); });
    run(p + ".wsola", [&] { put(p + ".wsola.out", d.warp(tgts, idx, 7)); });
    run(p + ".wsola_spans", [&] { put(p + ".wsola_spans.out", d.warp_spans(tgts, spots, 7)); });
}

static void all_calls()
{
    const Sounds recs = sounds_of("rec"), tgts = sounds_of("tgt"), segs = sounds_of("seg"), repl = sounds_of("repl");
    auto ctx = std::make_shared<Context>(SSYM_METRIC_DTW);
    SoundDictionary S(ctx), R(ctx);
    S.sounds = segs;
    R.sounds = recs;
    const std::vector<double> &dist = in("distances").f;
    const std::vector<uint32_t> &ia = in("indices.a").u, &ib = in("indices.b").u, &si = in("spot.indices").u;

    // a. match_indices_step
    run("a.paced", [&] { put("a.paced.idx", S.match_indices_step(tgts, nullptr, SSYM_STEP_PACED)); });
    run("a.paced.costs", [&] {
        std::vector<double> c;
        put("a.paced.costs.idx", S.match_indices_step(tgts, nullptr, SSYM_STEP_PACED, &c));
        put("a.paced.costs.cost", c);
    });
    run("a.paced.dist", [&] { put("a.paced.dist.idx", S.match_indices_step(tgts, dist.data(), SSYM_STEP_PACED)); });
    run("a.paced.dist.costs", [&] {
        std::vector<double> c;
        put("a.paced.dist.costs.idx", S.match_indices_step(tgts, dist.data(), SSYM_STEP_PACED, &c));
        put("a.paced.dist.costs.cost", c);
    });
    run("a.sym", [&] {
        std::vector<double> c;
        put("a.sym.idx", S.match_indices_step(tgts, dist.data(), SSYM_STEP_SYMMETRIC, &c));
        put("a.sym.cost", c);
        put("a.sym.match_indices", S.match_indices(tgts, dist.data()));
    });
    // b. pair_matrix_step: 6 segments x targets 1 ... 5
    const Sounds five(tgts.begin() + 1, tgts.end());
    for (uint32_t step : STEPS)
        run(std::string("b.") + step_name(step), [&] { put(std::string("b.") + step_name(step) + ".out", S.pair_matrix_step(five, step)); });
    // c. candidates
    for (uint32_t k : {1u, 3u, 9u})
        run("c.k" + std::to_string(k), [&] { put_sound_lists("c.k" + std::to_string(k), S.candidates(tgts, k, dist.data()), S); });
    run("c.plain", [&] { put_sound_lists("c.plain", S.candidates(tgts, 3), S); });
    // d. chain_indices
    run("d.chain", [&] { put("d.chain.idx", S.chain_indices(*tgts[3], in("chain.distances").f)); });
    // e. align, f. warp
    for (const char *which : {"a", "b"}) {
        const std::vector<uint32_t> &idx = which[0] == 'a' ? ia : ib;
        for (uint32_t step : STEPS) {
            const std::string name = std::string("e.") + step_name(step) + "." + which;
            run(name, [&] { put_alignments(name, S.align(tgts, idx, step)); });
        }
        for (uint32_t search : {0u, 7u, 512u}) {
            const std::string name = "f.s" + std::to_string(search) + "." + which;
            run(name, [&] { put(name + ".out", S.warp(tgts, idx, search)); });
        }
    }
    // g. spot, h. spot_all; their results feed i.
    std::map<std::string, std::vector<Spot>> fed;
    for (uint32_t step : STEPS) {
        const std::string s = step_name(step);
        run("g." + s, [&] { put_spots("g." + s, fed["g." + s] = R.spot(tgts, nullptr, step)); });
        run("g." + s + ".idx", [&] { put_spots("g." + s + ".idx", fed["g." + s + ".idx"] = R.spot(tgts, &si, step)); });
    }
    for (uint32_t k : {1u, 8u, 64u})
        run("h.sym.k" + std::to_string(k), [&] {
            const auto lists = R.spot_all(tgts, nullptr, k);
            put_spot_lists("h.sym.k" + std::to_string(k), lists);
            if (k == 8)
                fed["h.sym"] = heads(lists);
        });
    run("h.paced.k8", [&] {
        const auto lists = R.spot_all(tgts, nullptr, 8, nullptr, SSYM_STEP_PACED);
        put_spot_lists("h.paced.k8", lists);
        fed["h.paced"] = heads(lists);
    });
    run("h.sym.idx", [&] { put_spot_lists("h.sym.idx", R.spot_all(tgts, &si, 8)); });
    run("h.paced.idx", [&] { put_spot_lists("h.paced.idx", R.spot_all(tgts, &si, 8, nullptr, SSYM_STEP_PACED)); });
    const double limit = in("spot_all.max_cost").f.at(0);
    run("h.sym.max_cost", [&] { put_spot_lists("h.sym.max_cost", R.spot_all(tgts, nullptr, 8, &limit)); });
    run("h.sym.idx.max_cost", [&] { put_spot_lists("h.sym.idx.max_cost", R.spot_all(tgts, &si, 8, &limit)); });
    // i. align_spans, warp_spans
    {
        std::vector<Spot> hand;
        const auto &hs = in("hand.src").u, &ha = in("hand.start").u, &hb = in("hand.end").u;
        for (size_t t = 0; t < hs.size(); ++t)
            hand.push_back(hs[t] == SSYM_NO_MATCH ? no_spot() : Spot{hs[t], ha[t], hb[t], 0.0});
        for (uint32_t step : STEPS) {
            const std::string s = step_name(step);
            const std::pair<const char *, std::vector<Spot>> sets[4] = {
                {"spot", fed["g." + s]}, {"spot.idx", fed["g." + s + ".idx"]}, {"heads", fed["h." + s]}, {"hand", hand}};
            for (const auto &set : sets) {
                const std::string name = "i." + s + "." + set.first;
                if (set.second.size() != tgts.size()) {      // the call that was to give them threw: recorded there
                    put(name + ".code", std::vector<double>{9998.0});
                    continue;
                }
                run(name, [&] {
                    put_alignments(name + ".align", R.align_spans(tgts, set.second, step));
                    put(name + ".warp.s0", R.warp_spans(tgts, set.second, 0, step));
                    put(name + ".warp.s64", R.warp_spans(tgts, set.second, 64, step));
                });
            }
        }
    }
    // j. Spotter
    {
        const std::vector<double> &mc = in("spotter.max_cost").f;
        const std::vector<uint32_t> &lanes3 = in("lanes3").u;
        for (uint32_t step : STEPS)
            for (int limited = 0; limited < 2; ++limited) {
                const std::string tail = std::string(".") + step_name(step) + (limited ? ".max_cost" : ".free");
                run("j.l1" + tail, [&] { spotter_case("j.l1" + tail, ctx, tgts, recs, {0}, in("push1").w, 0, limited ? &mc : nullptr, step); });
                run("j.l3" + tail, [&] { spotter_case("j.l3" + tail, ctx, tgts, recs, lanes3, in("push3").w, 1, limited ? &mc : nullptr, step); });
            }
        // follow: a two-lane stream fed the samples of recordings 0 and 1 in blocks
        run("j.follow", [&] {
            ssym_stream *st = nullptr;
            ctx->check(ssym_stream_create(ctx->get(), 2, 44100.0, (uint32_t)NCOEFFS, 100.0, 8000.0, 0, &st));
            try {
                Spotter sp(ctx, tgts, 2);
                const std::vector<uint64_t> &blocks = in("follow").w;
                uint64_t done[2] = {0, 0};
                for (size_t k = 0; k < blocks.size() / 2; ++k) {
                    std::vector<double> smp;
                    std::vector<uint64_t> off{0};
                    for (int l = 0; l < 2; ++l) {
                        const auto &x = recs[l]->samples();
                        smp.insert(smp.end(), x.begin() + (std::ptrdiff_t)done[l], x.begin() + (std::ptrdiff_t)(done[l] + blocks[2 * k + l]));
                        done[l] += blocks[2 * k + l];
                        off.push_back(smp.size());
                    }
                    ctx->check(ssym_stream_push(ctx->get(), st, smp.data(), off.data(), 0, nullptr, nullptr));
                    const std::string q = "j.follow.push" + std::to_string(k);
                    put_events(q, sp.follow(st));
                    put_spots(q + ".best", sp.best());
                    put(q + ".counts", sp.counts());
                }
                for (uint32_t l = 0; l < 2; ++l)
                    put_events("j.follow.flush" + std::to_string(l), sp.flush(l));
            } catch (...) {
                ssym_stream_destroy(ctx->get(), st);
                throw;
            }
            ssym_stream_destroy(ctx->get(), st);
        });
    }
    // l. refusals that depend on the arguments
    {
        const std::vector<uint32_t> five_idx(5, 0), outside{0, 1, 99, 2, 4, 3};
        const std::vector<Spot> five_spots(5, Spot{0, 0, 0, 0.0}), good(6, Spot{0, 0, 5, 0.0});
        std::vector<Spot> beyond = good, outside_spots = good;
        beyond[2] = Spot{1, 60, 70, 0.0};                 // recording 1 has frames 0 ... 69
        outside_spots[2] = Spot{99, 0, 5, 0.0};
        const std::vector<double> five_costs(5, 1.0);
        run("l.align.length", [&] { S.align(tgts, five_idx); });
        run("l.align.length.paced", [&] { S.align(tgts, five_idx, SSYM_STEP_PACED); });
        run("l.align.length.none", [&] { S.align({}, five_idx); });      // (no targets, and indices all the same)
        run("l.warp.length", [&] { S.warp(tgts, five_idx); });
        run("l.spot.length", [&] { R.spot(tgts, &five_idx); });
        run("l.spot.length.paced", [&] { R.spot(tgts, &five_idx, SSYM_STEP_PACED); });
        run("l.spot_all.length", [&] { R.spot_all(tgts, &five_idx); });
        run("l.align_spans.length", [&] { R.align_spans(tgts, five_spots); });
        run("l.warp_spans.length", [&] { R.warp_spans(tgts, five_spots); });
        run("l.spotter.max_cost.length", [&] { Spotter sp(ctx, tgts, 1, &five_costs); });
        run("l.spotter.frame_offsets.length", [&] {
            Spotter sp(ctx, tgts, 3);
            sp.push(std::vector<double>(NCOEFFS, 0.0), {0, 1, 1});
        });
        run("l.align.outside", [&] { S.align(tgts, outside); });
        run("l.warp.outside", [&] { S.warp(tgts, outside); });
        run("l.spot.outside", [&] { R.spot(tgts, &outside); });
        run("l.spot_all.outside", [&] { R.spot_all(tgts, &outside); });
        run("l.align_spans.outside", [&] { R.align_spans(tgts, outside_spots); });
        run("l.warp_spans.outside", [&] { R.warp_spans(tgts, outside_spots); });
        run("l.align_spans.beyond", [&] { R.align_spans(tgts, beyond); });
        run("l.warp_spans.beyond", [&] { R.warp_spans(tgts, beyond); });
        run("l.warp.search513", [&] { S.warp(tgts, ia, 513); });
        run("l.warp_spans.search513", [&] { R.warp_spans(tgts, good, 513); });
        run("l.spot_all.max_spots0", [&] { R.spot_all(tgts, nullptr, 0); });
        run("l.spot_all.max_spots65", [&] { R.spot_all(tgts, nullptr, 65); });
        run("l.spot_all.idx.max_spots0", [&] { R.spot_all(tgts, &si, 0); });
        run("l.spot_all.idx.max_spots65", [&] { R.spot_all(tgts, &si, 65); });
        run("l.flush.lane", [&] {
            Spotter sp(ctx, tgts, 2);
            sp.flush(2);
        });
        run("l.reset.lane", [&] {
            Spotter sp(ctx, tgts, 2);
            sp.reset(2);
        });
    }
    // ... every method on a refcos context, and on an empty dictionary
    {
        auto rctx = std::make_shared<Context>(SSYM_METRIC_REFCOS);
        SoundDictionary RR(rctx);
        RR.sounds = recs;
        every_method("l.refcos", rctx, RR, tgts, true);
        SoundDictionary E(ctx);
        every_method("l.empty", ctx, E, tgts, false);
        run("l.empty.chain", [&] { E.chain_indices(*tgts[3], in("chain.distances").f); });
        run("l.empty.empty", [&] { E.align({}, {}); });          // no sounds and no targets: the dictionary is asked first
    }
    // m. an empty target list through every method
    every_method("m", ctx, R, {}, true);
    // k. an entry replaced in place (same length): the resident copy follows the content
    R.sounds[0] = repl[0];
    S.sounds[2] = repl[1];
    run("k.spot", [&] { put_spots("k.spot", R.spot(tgts)); });
    run("k.spot.paced", [&] { put_spots("k.spot.paced", R.spot(tgts, nullptr, SSYM_STEP_PACED)); });
    run("k.align", [&] { put_alignments("k.align", S.align(tgts, ia)); });
    run("k.warp_spans", [&] { put("k.warp_spans.out", R.warp_spans(tgts, R.spot(tgts), 0)); });
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::printf("usage: %s <case file> <result file>\n", argv[0]);
        return 2;
    }
    if (!read_arrays(argv[1])) {
        std::printf("%s: not a case file\n", argv[1]);
        return 2;
    }
    try {
        all_calls();
    } catch (const std::exception &e) {
        std::printf("outside every call: %s\n", e.what());
        ++g_bad;
    }
    if (!write_arrays(argv[2])) {
        std::printf("%s: cannot write\n", argv[2]);
        return 2;
    }
    std::printf(g_bad ? "%d calls ended in something else than a soundsym::Error\n" : "every call returned or threw a soundsym::Error\n", g_bad);
    return g_bad ? 1 : 0;
}
