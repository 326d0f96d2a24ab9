// tests/cpp/test_mirror_follow.cpp -- envelope following in the C++ mirror (include/soundsym.hpp): follow_envelope on a packed
// batch, and warp / warp_spans with Dynamics::Target, run on the sounds of tests/mirror_cases.py; the results are written out
// for tests/test_gpu_mirror_follow.py to compare with the Python layer's on the same sounds.
//
//   test_mirror_follow <case file> <result file>
//
// Both files are the container of tests/mirror_cases.py, read and written as tests/cpp/test_mirror_resynth.cpp does it (the
// same text).  The program asserts nothing about values.  Every call runs inside run(name, ...), which records
// "<name>.code": 0 when the call returned, the exception's code when it threw a soundsym::Error.
//
// Build: tests/cpp/follow.mk.
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
using Spot = SoundDictionary::Spot;

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

static void all_calls()
{
    const Sounds recs = sounds_of("rec"), tgts = sounds_of("tgt"), segs = sounds_of("seg");
    auto ctx = std::make_shared<Context>(SSYM_METRIC_DTW);
    auto rctx = std::make_shared<Context>(SSYM_METRIC_REFCOS);
    const std::vector<double> &y = in("follow.samples").f, &x = in("follow.ref").f, &max_gains = in("follow.max_gains").f;
    const std::vector<uint64_t> &off = in("follow.off").w, &r_off = in("follow.r_off").w;
    // a. follow_envelope on the packed batch at every max_gain, with and without the gains; on a refcos context too
    for (size_t k = 0; k < max_gains.size(); ++k) {
        const std::string name = "a.g" + std::to_string(k);
        run(name, [&] {
            std::vector<double> gains;
            put(name + ".out", follow_envelope(*ctx, y, off, x, r_off, max_gains[k], &gains));
            put(name + ".gains", gains);
        });
    }
    run("a.default", [&] { put("a.default.out", follow_envelope(*ctx, y, off, x, r_off)); });
    run("a.refcos", [&] { put("a.refcos.out", follow_envelope(*rctx, y, off, x, r_off, max_gains[0])); });
    run("a.none", [&] {
        std::vector<double> gains{1.0, 2.0};
        put("a.none.out", follow_envelope(*ctx, {}, {0}, {}, {0}, 8.0, &gains));
        put("a.none.gains", gains);
    });
    // b. warp and warp_spans with the dynamics argument, and without it
    SoundDictionary S(ctx), R(ctx);
    S.sounds = segs;
    R.sounds = recs;
    const std::vector<uint32_t> &ia = in("indices.a").u;
    const auto &hs = in("hand.src").u, &ha = in("hand.start").u, &hb = in("hand.end").u;
    std::vector<Spot> hand;
    for (size_t t = 0; t < hs.size(); ++t)
        hand.push_back(hs[t] == SSYM_NO_MATCH ? Spot{SSYM_NO_MATCH, SSYM_NO_MATCH, SSYM_NO_MATCH, std::numeric_limits<double>::infinity()}
                                              : Spot{hs[t], ha[t], hb[t], 0.0});
    for (uint32_t search : {0u, 16u}) {
        const std::string s = ".s" + std::to_string(search);
        run("b.warp" + s, [&] { put("b.warp" + s + ".out", S.warp(tgts, ia, search, Dynamics::Target)); });
        run("b.warp.g2" + s, [&] { put("b.warp.g2" + s + ".out", S.warp(tgts, ia, search, Dynamics::Target, 2.0)); });
        run("b.warp.plain" + s, [&] { put("b.warp.plain" + s + ".out", S.warp(tgts, ia, search, Dynamics::None, 2.0)); });
        run("b.spans" + s, [&] { put("b.spans" + s + ".out", R.warp_spans(tgts, hand, search, SSYM_STEP_SYMMETRIC, Dynamics::Target)); });
        run("b.spans.plain" + s, [&] { put("b.spans.plain" + s + ".out", R.warp_spans(tgts, hand, search)); });
    }
    run("b.spans.paced", [&] { put("b.spans.paced.out", R.warp_spans(tgts, hand, 0, SSYM_STEP_PACED, Dynamics::Target, 3.0)); });
    // l. refusals
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    run("l.gain.low", [&] { follow_envelope(*ctx, y, off, x, r_off, 0.5); });
    run("l.gain.nan", [&] { follow_envelope(*ctx, y, off, x, r_off, nan); });
    run("l.gain.inf", [&] { follow_envelope(*ctx, y, off, x, r_off, inf); });
    run("l.offsets.count", [&] { follow_envelope(*ctx, y, off, x, std::vector<uint64_t>(r_off.begin(), r_off.end() - 1)); });
    run("l.offsets.none", [&] { follow_envelope(*ctx, y, {}, x, {}); });
    run("l.offsets.start", [&] {
        std::vector<uint64_t> bad(off);
        bad[0] = 1;
        follow_envelope(*ctx, y, bad, x, r_off);
    });
    run("l.offsets.decrease", [&] {
        std::vector<uint64_t> bad(r_off);
        std::swap(bad[1], bad[2]);
        follow_envelope(*ctx, y, off, x, bad);
    });
    run("l.samples.short", [&] { follow_envelope(*ctx, std::vector<double>(y.begin(), y.end() - 1), off, x, r_off); });
    run("l.warp.gain", [&] { S.warp(tgts, ia, 0, Dynamics::Target, 0.5); });
    run("l.warp.gain.unused", [&] { S.warp(tgts, ia, 0, Dynamics::None, nan); });
    run("l.spans.gain", [&] { R.warp_spans(tgts, hand, 0, SSYM_STEP_SYMMETRIC, Dynamics::Target, inf); });
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
