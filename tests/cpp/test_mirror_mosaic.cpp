// tests/cpp/test_mirror_mosaic.cpp -- SoundDictionary::mosaic of the C++ mirror (include/soundsym.hpp) run on the planted
// intruder case of tests/mosaic_ref.py, the results written out for tests/test_gpu_mirror_mosaic.py to compare, call for
// call, with the Python mirror's on the same sounds.
//
//   test_mirror_mosaic <case file> <result file>
//
// Both files are the container of tests/mirror_cases.py, read and written as tests/cpp/test_mirror_cover.cpp does it (the
// same text).  The program asserts nothing about values.  Every call runs inside run(name, ...), which records
// "<name>.code": 0 when the call returned, the exception's code when it threw a soundsym::Error.
//
// Build: tests/cpp/mosaic.mk.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>

#include "soundsym.hpp"

using namespace soundsym;
using Mosaic = SoundDictionary::Mosaic;
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

// the mosaics of one call: tiles per mosaic (offsets), the tiles (a gap has the source SSYM_COVER_GAP), every tile's
// frame_map (offsets per tile), the totals and the frame costs (offsets per mosaic)
static void put_mosaics(const std::string &p, const std::vector<Mosaic> &mosaics)
{
    std::vector<uint64_t> off{0}, map_off{0}, fc_off{0};
    std::vector<uint32_t> src, first, last, start, end, map;
    std::vector<double> cost, total, fc;
    for (const auto &m : mosaics) {
        for (const auto &piece : m.pieces) {
            src.push_back(piece.source_index);
            first.push_back(piece.source_first);
            last.push_back(piece.source_last);
            start.push_back(piece.start_frame);
            end.push_back(piece.end_frame);
            cost.push_back(piece.cost);
            map.insert(map.end(), piece.frame_map.begin(), piece.frame_map.end());
            map_off.push_back(map.size());
        }
        off.push_back(src.size());
        total.push_back(m.total);
        fc.insert(fc.end(), m.frame_costs.begin(), m.frame_costs.end());
        fc_off.push_back(fc.size());
    }
    put(p + ".off", off);
    put(p + ".src", src);
    put(p + ".first", first);
    put(p + ".last", last);
    put(p + ".start", start);
    put(p + ".end", end);
    put(p + ".cost", cost);
    put(p + ".map", map);
    put(p + ".map_off", map_off);
    put(p + ".total", total);
    put(p + ".fc", fc);
    put(p + ".fc_off", fc_off);
}

static void all_calls()
{
    auto ctx = std::make_shared<Context>(SSYM_METRIC_DTW);
    const Sounds tgts = sounds_of("tgt"), segs = sounds_of("seg");
    const std::vector<double> &penalties = in("penalties").f, &gaps = in("gaps").f;
    SoundDictionary S(ctx);
    S.sounds = segs;
    // a. every (penalty, gap_cost), +inf among the gap costs; then the call without a gap_cost
    for (size_t k = 0; k < penalties.size(); ++k)
        for (size_t g = 0; g < gaps.size(); ++g) {
            const std::string name = "a.p" + std::to_string(k) + ".g" + std::to_string(g);
            run(name, [&] { put_mosaics(name, S.mosaic(tgts, penalties[k], gaps[g])); });
        }
    run("a.plain", [&] { put_mosaics("a.plain", S.mosaic(tgts, penalties[0])); });
    // b. one target at a time
    for (size_t t = 0; t < tgts.size(); ++t)
        run("b.t" + std::to_string(t), [&] { put_mosaics("b.t" + std::to_string(t), S.mosaic({tgts[t]}, penalties[0], gaps[0])); });
    // l. refusals: a gap_cost or a penalty that is none, a refcos context, no dictionary
    SoundDictionary E(ctx);
    run("l.negative", [&] { S.mosaic(tgts, 0.0, -1.0); });
    run("l.nan", [&] { S.mosaic(tgts, 0.0, std::numeric_limits<double>::quiet_NaN()); });
    run("l.ninf", [&] { S.mosaic(tgts, 0.0, -std::numeric_limits<double>::infinity()); });
    run("l.penalty", [&] { S.mosaic(tgts, -1.0, 1.0); });
    run("l.empty", [&] { E.mosaic(tgts, 0.0, 1.0); });
    auto rctx = std::make_shared<Context>(SSYM_METRIC_REFCOS);
    SoundDictionary RR(rctx);
    RR.sounds = segs;
    run("l.refcos", [&] { RR.mosaic(tgts, 0.0, 1.0); });
    // m. no targets
    run("m", [&] { put_mosaics("m", S.mosaic({}, 0.0, 1.0)); });
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
