// tests/cpp/test_mirror_follower.cpp -- live envelope following in the C++ mirror (include/soundsym.hpp class Follower): three
// lanes fed the signals of the case file in the cuts it names, one lane reset, every lane flushed; every call's samples, pcm,
// gains and offsets and the counts are written out for tests/test_gpu_mirror_follower.py to compare with the Python layer's
// (Engine.follower) on the same calls.
//
//   test_mirror_follower <case file> <result file>
//
// Both files are the container of tests/mirror_cases.py, read and written as tests/cpp/test_mirror_follow.cpp does it (the
// same text).  The program asserts nothing about values.  Every call runs inside run(name, ...), which records
// "<name>.code": 0 when the call returned, the exception's code when it threw a soundsym::Error.
//
// Build: tests/cpp/follower.mk.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <memory>

#include "soundsym.hpp"

using namespace soundsym;

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

static std::vector<double> widen(const std::vector<uint64_t> &v) { return std::vector<double>(v.begin(), v.end()); }
static std::vector<double> widen(const std::vector<int32_t> &v) { return std::vector<double>(v.begin(), v.end()); }

static void put(const std::string &name, const Follower::Samples &s)
{
    put(name + ".off", widen(s.lane_offsets));
    put(name + ".out", s.samples);
    put(name + ".pcm", widen(s.pcm32));
    put(name + ".g_off", widen(s.gain_offsets));
    put(name + ".gains", s.gains);
}

static void all_calls()
{
    auto ctx = std::make_shared<Context>(SSYM_METRIC_DTW);
    auto rctx = std::make_shared<Context>(SSYM_METRIC_REFCOS);
    const std::vector<double> &y = in("follower.samples").f, &x = in("follower.ref").f;
    const std::vector<uint64_t> &off = in("follower.off").w, &r_off = in("follower.r_off").w;     // the lanes' whole signals
    const std::vector<uint64_t> &y_cuts = in("follower.y_cuts").w, &x_cuts = in("follower.x_cuts").w;
    const uint32_t lanes = (uint32_t)off.size() - 1, reset_lane = in("follower.reset").u[0], reset_after = in("follower.reset").u[1];
    const double max_gain = in("follower.max_gain").f[0];
    // a. the lanes in cuts: push p gives lane l its samples [cut[p], cut[p + 1]) (clipped to its length); one lane is reset on the
    // way and goes on with the later slices as a new signal; the flushes
    for (const auto &which : {std::make_pair(std::string("a"), ctx), std::make_pair(std::string("r"), rctx)}) {
        const std::string tag = which.first;
        std::unique_ptr<Follower> fl;
        run(tag + ".create", [&] { fl = std::make_unique<Follower>(which.second, lanes, max_gain); });
        if (!fl)
            continue;
        for (size_t p = 0; p + 1 < y_cuts.size(); ++p) {
            std::vector<double> ys, xs;
            std::vector<uint64_t> yo{0}, xo{0};
            for (uint32_t l = 0; l < lanes; ++l) {
                const uint64_t n = off[l + 1] - off[l], nx = r_off[l + 1] - r_off[l];
                const uint64_t ya = y_cuts[p], yb = y_cuts[p + 1], xa = x_cuts[p], xb = x_cuts[p + 1];
                ys.insert(ys.end(), y.begin() + off[l] + std::min(ya, n), y.begin() + off[l] + std::min(yb, n));
                xs.insert(xs.end(), x.begin() + r_off[l] + std::min(xa, nx), x.begin() + r_off[l] + std::min(xb, nx));
                yo.push_back(ys.size());
                xo.push_back(xs.size());
            }
            const std::string name = tag + ".push" + std::to_string(p);
            run(name, [&] { put(name, fl->push(ys, yo, xs, xo)); });
            if (p == reset_after)
                run(tag + ".reset", [&] { fl->reset(reset_lane); });
        }
        run(tag + ".counts", [&] {
            const Follower::Counts c = fl->counts();
            put(tag + ".counts.ny", widen(c.ny));
            put(tag + ".counts.nx", widen(c.nx));
            put(tag + ".counts.released", widen(c.released));
        });
        for (uint32_t l = 0; l < lanes; ++l) {
            const std::string name = tag + ".flush" + std::to_string(l);
            run(name, [&] { put(name, fl->flush(l)); });
        }
    }
    // b. one lane, the bare signals, the default max_gain
    run("b", [&] {
        Follower one(ctx);
        const std::vector<double> y0(y.begin() + off[0], y.begin() + off[1]), x0(x.begin() + r_off[0], x.begin() + r_off[1]);
        put("b.push", one.push(y0, x0));
        put("b.flush", one.flush());
    });
    // l. refusals
    const double nan = std::numeric_limits<double>::quiet_NaN();
    run("l.gain.low", [&] { Follower f(ctx, 1, 0.5); });
    run("l.gain.nan", [&] { Follower f(ctx, 1, nan); });
    run("l.lanes.none", [&] { Follower f(ctx, 0); });
    run("l.lanes.many", [&] { Follower f(ctx, 16385); });
    Follower f(ctx, 2);
    run("l.offsets.count", [&] { f.push({1.0}, {0, 1}, {}, {0, 0, 0}); });
    run("l.offsets.start", [&] { f.push({1.0, 2.0}, {1, 1, 2}, {}, {0, 0, 0}); });
    run("l.offsets.decrease", [&] { f.push({1.0, 2.0}, {0, 2, 1}, {}, {0, 0, 0}); });
    run("l.samples.short", [&] { f.push({1.0}, {0, 1, 2}, {}, {0, 0, 0}); });
    run("l.lane.outside", [&] { f.flush(2); });
    run("l.reset.outside", [&] { f.reset(2); });
    run("l.flush.ok", [&] { f.flush(1); });
    run("l.lane.ended", [&] { f.flush(1); });
    run("l.push.ended", [&] { f.push({1.0}, {0, 0, 1}, {}, {0, 0, 0}); });
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
