// tests/cpp/test_mirror_resynth.cpp -- the Resynth of the C++ mirror (include/soundsym.hpp) run on sounds of
// tests/mirror_cases.py behind a Mosaicker, the results written out for tests/test_gpu_mirror_resynth.py to compare, call for
// call, with the Python Resynth's on the same sounds.
//
//   test_mirror_resynth <case file> <result file>
//
// Both files are the container of tests/mirror_cases.py, read and written as tests/cpp/test_mirror_mosaicker.cpp does it (the
// same text).  The program asserts nothing about values.  Every call runs inside run(name, ...), which records
// "<name>.code": 0 when the call returned, the exception's code when it threw a soundsym::Error.
//
// Build: tests/cpp/resynth.mk.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>

#include "soundsym.hpp"

using namespace soundsym;
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

// the frames of one call
static void put_frames(const std::string &p, const std::vector<Mosaicker::Frame> &frames)
{
    std::vector<uint32_t> lane, column, src, frame, start;
    std::vector<double> cost;
    for (const auto &x : frames) {
        lane.push_back(x.lane);
        column.push_back(x.column);
        src.push_back(x.src);
        frame.push_back(x.frame);
        cost.push_back(x.cost);
        start.push_back(x.start ? 1u : 0u);
    }
    put(p + ".lane", lane);
    put(p + ".column", column);
    put(p + ".src", src);
    put(p + ".frame", frame);
    put(p + ".cost", cost);
    put(p + ".start", start);
}

// the samples of one call; the 32-bit samples go out as their u32 bits
static void put_samples(const std::string &p, const Resynth::Samples &s)
{
    put(p + ".offsets", s.lane_offsets);
    put(p + ".samples", s.samples);
    put(p + ".pcm", std::vector<uint32_t>(s.pcm32.begin(), s.pcm32.end()));
}

static void all_calls()
{
    auto ctx = std::make_shared<Context>(SSYM_METRIC_DTW);
    const Sounds segs = sounds_of("seg"), recs = sounds_of("rec");
    const std::vector<double> &penalties = in("penalties").f;
    const double gap = in("mosaicker.gap").f[0];
    const size_t block = (size_t)in("mosaicker.block").w[0], n_lanes = (size_t)in("mosaicker.lanes").w[0];
    const uint32_t search = (uint32_t)in("resynth.search").w[0];
    // a. the first recordings as lanes of a mosaicker, pushed block by block, then flushed; the dictionary is every segment,
    // uncut, and so is the sample store of the two resynthesisers: R with a search, P the plain warp
    Mosaicker M(ctx, segs, (uint32_t)n_lanes, penalties[1], gap);
    Resynth R(ctx, segs, (uint32_t)n_lanes, search), P(ctx, segs, (uint32_t)n_lanes, 0);
    size_t longest = 0;
    for (size_t l = 0; l < n_lanes; ++l)
        longest = std::max<size_t>(longest, recs[l]->num_frames());
    size_t pushes = 0;
    for (size_t at = 0; at < longest; at += block, ++pushes) {
        std::vector<double> feats;
        std::vector<uint64_t> off{0};
        for (size_t l = 0; l < n_lanes; ++l) {
            const std::vector<double> &m = recs[l]->mfccs();
            const size_t frames = recs[l]->num_frames(), lo = std::min(at, frames), hi = std::min(at + block, frames);
            feats.insert(feats.end(), m.begin() + lo * NCOEFFS, m.begin() + hi * NCOEFFS);
            off.push_back(off.back() + (hi - lo));
        }
        // every frame log is taken device to device by R and pushed as host rows into P
        const std::string name = "a.push" + std::to_string(pushes);
        std::vector<Mosaicker::Frame> frames;
        run(name, [&] { put_frames(name, frames = M.push(feats, off)); });
        run(name + ".take", [&] { put_samples(name + ".take", R.take(M)); });
        run(name + ".rows", [&] { put_samples(name + ".rows", P.push(frames)); });
    }
    put("a.pushes", std::vector<uint64_t>{pushes});
    run("a.counts", [&] { put("a.counts", R.counts()); });
    run("a.released", [&] { put("a.released", R.released()); });
    for (size_t l = n_lanes; l-- > 0;) {
        const std::string name = "a.flush" + std::to_string(l);
        const uint64_t total = (uint64_t)recs[l]->num_frames() * 256 + 100;
        std::vector<Mosaicker::Frame> frames;
        run(name, [&] { put_frames(name, frames = M.flush((uint32_t)l)); });
        run(name + ".take", [&] { put_samples(name + ".take", R.take(M)); });
        run(name + ".rows", [&] { put_samples(name + ".rows", P.push(frames)); });
        run(name + ".end", [&] { put_samples(name + ".end", R.flush((uint32_t)l, total)); });
        run(name + ".rows.end", [&] { put_samples(name + ".rows.end", P.flush((uint32_t)l, total)); });
    }
    run("a.released.end", [&] { put("a.released.end", R.released()); });
    // b. a lane that has ended takes no frames until it is reset; then it starts again
    const std::vector<Resynth::Frame> rows{{0, 0, 1, 3, true}, {0, 1, 1, 4, false}, {0, 2, SSYM_COVER_GAP, SSYM_NO_MATCH, true}};
    run("b.ended", [&] { P.push(rows); });
    run("b.reset", [&] { P.reset(0); });
    run("b.again", [&] { put_samples("b.again", P.push(rows)); });
    run("b.flush", [&] { put_samples("b.flush", P.flush(0, 3 * 256 + 77)); });
    run("b.counts", [&] { put("b.counts", P.counts()); });
    // l. refusals
    run("l.twice", [&] { R.take(M); });
    run("l.lane", [&] { P.flush((uint32_t)n_lanes, 0); });
    run("l.reset", [&] { P.reset((uint32_t)n_lanes); });
    run("l.short", [&] { P.reset(0); P.push(rows); P.flush(0, 3 * 256 - 1); });
    run("l.column", [&] { P.push(std::vector<Resynth::Frame>{{0, 7, 1, 3, true}}); });
    run("l.step", [&] { P.push(std::vector<Resynth::Frame>{{0, 3, SSYM_COVER_GAP, SSYM_NO_MATCH, false}}); });
    run("l.src", [&] { P.push(std::vector<Resynth::Frame>{{0, 3, (uint32_t)segs.size(), 0, true}}); });
    run("l.search", [&] { Resynth x(ctx, segs, 1, 513); });
    run("l.lanes", [&] { Resynth x(ctx, segs, 0); });
    run("l.empty", [&] { Resynth x(ctx, Sounds{}); });
    auto rctx = std::make_shared<Context>(SSYM_METRIC_REFCOS);
    run("l.refcos", [&] { Resynth x(rctx, segs, 1, 16); put_samples("l.refcos", x.push(rows)); });
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
