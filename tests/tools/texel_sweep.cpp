// TEST INFRASTRUCTURE: the rgb8 texel of every float of a range, in the two forms the suite compares
// (tests/tools/texel_ref.py). Builds on the CPU restatement (oracle/rt_oracle.cpp,
// included) for the reference's form:
//   form 0, the contract (rt_texel.h, rt_api.h): pow((double)c, (double)(1 / 2.2f)), narrowed to
//           float, times 255.f, truncated; written out below;
//   form 1, the reference (main.cxx:39-45,77-85): oracle_epilogue_rgb8 over chunks, which calls
//           this host's powf at run time.
// The floats are walked by their words, first..last (both non-negative, in increasing order of value).
// Every input of pow is read from memory that the caller's arguments filled, and the exponent comes
// in as an argument, so no call is folded at compile time.
#include "../../oracle/rt_oracle.cpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>

namespace {

constexpr std::uint32_t CHUNK = 1u << 16;

inline float word_float(std::uint32_t w)
{
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}

inline float contract_product(float c, double g)
{
    return 255.f * static_cast<float>(std::pow(static_cast<double>(c), g));
}

struct step { std::uint32_t word, texel; };

struct found {
    std::vector<step> steps[2];           // the first float of each run of a new texel value
    std::uint64_t non_monotone[2] = {0, 0};
    std::vector<std::uint32_t> differ;    // floats whose two texels differ
};

} // namespace

struct texel_sweep_result {
    std::uint32_t n_steps[2];             // steps found (may exceed cap; only cap are stored)
    std::uint64_t non_monotone[2];        // neighbours a, a+1 with texel(a+1) < texel(a)
    std::uint32_t n_differ;               // floats whose two texels differ (may exceed cap)
};

// steps_word / steps_texel: [2][cap]; differ: [cap]. exponent: 1 / 2.2f as the caller computed it.
extern "C" int texel_sweep(std::uint32_t first, std::uint32_t last, float exponent, int threads, std::uint32_t cap,
                           std::uint32_t *steps_word, std::uint32_t *steps_texel, std::uint32_t *differ,
                           texel_sweep_result *res)
{
    if (first > last || last >= 0x7f800000u || threads < 1 || !steps_word || !steps_texel || !differ || !res)
        return RT_ERR_INVALID;
    threads = std::min(threads, 16);
    const double g = static_cast<double>(exponent);
    const std::uint64_t n = static_cast<std::uint64_t>(last) - first + 1;
    const std::uint64_t n_chunks = (n + CHUNK - 1) / CHUNK;
    std::atomic<std::uint64_t> next{0};
    std::mutex m;
    found all;
    auto worker = [&] {
        found mine;
        std::vector<float> in(CHUNK + 1);
        std::vector<std::uint8_t> ref(CHUNK + 1);
        for (;;) {
            const std::uint64_t k = next.fetch_add(1);
            if (k >= n_chunks) break;
            const std::uint64_t a = first + k * CHUNK, b = std::min<std::uint64_t>(a + CHUNK, static_cast<std::uint64_t>(last) + 1);
            // the chunk's floats, led by the float before it (the neighbour of its first)
            const std::uint64_t lead = a > first ? a - 1 : a;
            const std::uint32_t cnt = static_cast<std::uint32_t>(b - lead);
            for (std::uint32_t i = 0; i < cnt; ++i) in[i] = word_float(static_cast<std::uint32_t>(lead + i));
            oracle_epilogue_rgb8(in.data(), ref.data(), cnt);
            std::uint32_t prev[2] = {0, 0};
            for (std::uint32_t i = 0; i < cnt; ++i) {
                const std::uint32_t w = static_cast<std::uint32_t>(lead + i);
                const std::uint32_t t[2] = {static_cast<std::uint8_t>(contract_product(in[i], g)), ref[i]};
                const bool counted = lead + i >= a;   // the leading float only supplies prev
                if (counted) {
                    for (int f = 0; f < 2; ++f) {
                        const bool start = w == first;
                        if (start ? t[f] != 0 : t[f] > prev[f]) mine.steps[f].push_back({w, t[f]});
                        if (!start && t[f] < prev[f]) ++mine.non_monotone[f];
                    }
                    if (t[0] != t[1]) mine.differ.push_back(w);
                }
                prev[0] = t[0]; prev[1] = t[1];
            }
        }
        std::lock_guard<std::mutex> lock(m);
        for (int f = 0; f < 2; ++f) {
            all.steps[f].insert(all.steps[f].end(), mine.steps[f].begin(), mine.steps[f].end());
            all.non_monotone[f] += mine.non_monotone[f];
        }
        all.differ.insert(all.differ.end(), mine.differ.begin(), mine.differ.end());
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
    for (int f = 0; f < 2; ++f) {
        auto &s = all.steps[f];
        std::sort(s.begin(), s.end(), [](const step &x, const step &y) { return x.word < y.word; });
        res->n_steps[f] = static_cast<std::uint32_t>(s.size());
        res->non_monotone[f] = all.non_monotone[f];
        for (std::uint32_t i = 0; i < std::min<std::size_t>(cap, s.size()); ++i) {
            steps_word[f * cap + i] = s[i].word;
            steps_texel[f * cap + i] = s[i].texel;
        }
    }
    std::sort(all.differ.begin(), all.differ.end());
    res->n_differ = static_cast<std::uint32_t>(all.differ.size());
    for (std::uint32_t i = 0; i < std::min<std::size_t>(cap, all.differ.size()); ++i) differ[i] = all.differ[i];
    return RT_OK;
}

// The first float from `from` upward whose product 255.f * pow reaches 256 (beyond it the cast to uint8_t
// is undefined), per form: [0] the contract's product, [1] the reference's 255.f * powf(c, exponent).
extern "C" int texel_first_256(std::uint32_t from, float exponent, std::uint32_t *out)
{
    if (!out || from >= 0x7f800000u) return RT_ERR_INVALID;
    const double g = static_cast<double>(exponent);
    volatile float e = exponent;
    for (int f = 0; f < 2; ++f) {
        std::uint32_t w = from;
        for (; w < 0x7f800000u; ++w) {
            const float c = word_float(w);
            const float p = f == 0 ? contract_product(c, g) : 255.f * std::pow(c, static_cast<float>(e));
            if (p >= 256.f) break;
        }
        out[f] = w;
    }
    return RT_OK;
}
