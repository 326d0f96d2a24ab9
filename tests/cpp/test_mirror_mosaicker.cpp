// tests/cpp/test_mirror_mosaicker.cpp -- the Mosaicker of the C++ mirror (include/soundsym.hpp) run on sounds of
// tests/mirror_cases.py, the results written out for tests/test_gpu_mirror_mosaicker.py to compare, call for call, with the
// Python Mosaicker's on the same sounds.
//
//   test_mirror_mosaicker <case file> <result file>
//
// Both files are the container of tests/mirror_cases.py, read and written as tests/cpp/test_mirror_coverer.cpp does it (the
// same text).  The program asserts nothing about values.  Every call runs inside run(name, ...), which records
// "<name>.code": 0 when the call returned, the exception's code when it threw a soundsym::Error.
//
// Build: tests/cpp/mosaicker.mk.
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

static void put_best(const std::string &p, const Mosaicker &c)
{
    std::vector<double> total;
    std::vector<uint32_t> covered, committed;
    for (const auto &b : c.best()) {
        total.push_back(b.total);
        covered.push_back(b.covered);
        committed.push_back(b.committed);
    }
    put(p + ".total", total);
    put(p + ".covered", covered);
    put(p + ".committed", committed);
}

static void all_calls()
{
    auto ctx = std::make_shared<Context>(SSYM_METRIC_DTW);
    const Sounds segs = sounds_of("seg"), recs = sounds_of("rec");
    const std::vector<double> &penalties = in("penalties").f;
    const double gap = in("mosaicker.gap").f[0];
    const size_t block = (size_t)in("mosaicker.block").w[0], n_lanes = (size_t)in("mosaicker.lanes").w[0];
    // a. the first recordings as lanes, pushed block by block, then flushed; the dictionary is every segment, uncut
    Mosaicker M(ctx, segs, (uint32_t)n_lanes, penalties[1], gap);
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
        const std::string name = "a.push" + std::to_string(pushes);
        run(name, [&] { put_frames(name, M.push(feats, off)); });
        run(name + ".best", [&] { put_best(name + ".best", M); });
    }
    put("a.pushes", std::vector<uint64_t>{pushes});
    run("a.counts", [&] { put("a.counts", M.counts()); });
    run("a.capacity", [&] { put("a.capacity", std::vector<uint64_t>{M.capacity()}); });
    for (size_t l = n_lanes; l-- > 0;) {
        const std::string name = "a.flush" + std::to_string(l);
        run(name, [&] { put_frames(name, M.flush((uint32_t)l)); });
    }
    run("a.best", [&] { put_best("a.best", M); });
    // b. a lane that has ended takes no frames until it is reset; then it starts again
    const std::vector<double> &m0 = recs[1]->mfccs();
    std::vector<uint64_t> again{0, (uint64_t)recs[1]->num_frames()};
    again.resize(n_lanes + 1, again[1]);
    run("b.ended", [&] { M.push(m0, again); });
    run("b.reset", [&] { M.reset(0); });
    run("b.again", [&] { put_frames("b.again", M.push(m0, again)); });
    run("b.flush", [&] { put_frames("b.flush", M.flush(0)); });
    run("b.counts", [&] { put("b.counts", M.counts()); });
    // c. without gaps
    run("c.plain", [&] {
        Mosaicker P(ctx, segs, 1, penalties[1]);
        put_frames("c.plain", P.push(m0, std::vector<uint64_t>{0, (uint64_t)recs[1]->num_frames()}));
        put_frames("c.flush", P.flush(0));
    });
    // l. refusals
    run("l.lane", [&] { M.flush((uint32_t)n_lanes); });
    run("l.reset", [&] { M.reset((uint32_t)n_lanes); });
    run("l.offsets", [&] { M.push(m0, std::vector<uint64_t>{0}); });
    run("l.negative", [&] { Mosaicker x(ctx, segs, 1, -1.0); });
    run("l.nan", [&] { Mosaicker x(ctx, segs, 1, std::numeric_limits<double>::quiet_NaN()); });
    run("l.gap", [&] { Mosaicker x(ctx, segs, 1, 1.0, -2.0); });
    run("l.lanes", [&] { Mosaicker x(ctx, segs, 0); });
    run("l.empty", [&] { Mosaicker x(ctx, Sounds{}); });
    auto rctx = std::make_shared<Context>(SSYM_METRIC_REFCOS);
    run("l.refcos", [&] { Mosaicker x(rctx, segs); });
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
