// Host check of csrc/vq_scr_keys.h, the tracker a lane of the screened Dp = 256 sweep runs per sub-tile: streams of 32 .. 96
// sub-tiles x 16 values go through scr_start_clamp / scr_track_update the way the kernel feeds them, and the result is set
// against a sort of all (key, code) pairs of the stream:
//  * the three lowest keys are those of the sort, as a multiset;
//  * (I1) b1 < b2 => the decoded code of b1 is the code of the lowest key;
//  * (I2) b2 < b3 => the decoded codes of b1 and b2 are the codes of the two lowest keys (two different codes);
//  * every key is within 15 ulp of its value, keeps its sign, is never a NaN, and for one r the tag is monotone;
//  * a padding code's key (start value +inf, last sub-tile) is finite and at least 2^99.
// Data classes: random values, negative values, exact zeros (+0 and -0: subnormal keys), duplicates at the same r in
// different sub-tiles, duplicates inside one sub-tile, triples, descending runs (every sub-tile lowers the lowest), +inf
// padding in the last sub-tile, and mixtures.  Built with -fsanitize=address,undefined by tests/test_scr_keys_host.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vq_scr_keys.h"

static int fails = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (fails++ < 20) {                  \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

static uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}
static float from_bits(uint32_t b) {
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}
// distance in representable floats (sign-magnitude -> a line)
static int64_t ordinal(float v) {
    const uint32_t b = bits(v);
    return (b & 0x80000000u) ? -(int64_t)(b & 0x7FFFFFFFu) : (int64_t)b;
}

struct KeyCode {
    float key;
    int code;
};

enum Class { RANDOM, NEGATIVE, ZEROS, DUP_SAME_R, DUP_IN_SUBTILE, TRIPLES, DESCENDING, PADDING, MIXED, NCLASS };
static const char *kNames[NCLASS] = {"random", "negative", "zeros", "dup_same_r", "dup_in_subtile", "triples", "descending", "padding", "mixed"};

// one stream: nsub sub-tiles x 16 accumulator values of one lane; npad padding codes at the end of the last sub-tile
static void make_stream(int cls, std::mt19937 &rng, int nsub, std::vector<float> &v, int &npad) {
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    std::normal_distribution<float> nrm(0.0f, 1.0f);
    v.assign((size_t)nsub * 16, 0.0f);
    npad = 0;
    auto at = [&](int u, int r) -> float & { return v[(size_t)u * 16 + r]; };
    const float scale = std::ldexp(1.0f, (int)(rng() % 60) - 30);
    for (int u = 0; u < nsub; ++u)
        for (int r = 0; r < 16; ++r) {
            float x = (1000.0f + 300.0f * nrm(rng)) * scale;  // distances: mostly positive, a few thousand ulp apart
            if (cls == NEGATIVE || (cls == MIXED && (rng() & 1))) x = -std::fabs(x) * uni(rng);
            if (cls == DESCENDING) x = (float)(nsub - u) * 100.0f * scale + (float)r * scale * (uni(rng) - 0.5f);
            at(u, r) = x;
        }
    auto pick_u = [&]() { return (int)(rng() % (unsigned)nsub); };
    auto pick_r = [&]() { return (int)(rng() % 16u); };
    const float low = (cls == NEGATIVE) ? -2.0f * scale : -5000.0f * scale;  // below everything else of the stream
    if (cls == ZEROS || cls == MIXED) {
        // everything else positive, zeros of both signs as the lowest values
        if (cls == ZEROS)
            for (auto &x : v) x = std::fabs(x) + scale;
        const int n = 1 + (int)(rng() % 4u);
        for (int i = 0; i < n; ++i) at(pick_u(), pick_r()) = (rng() & 1) ? 0.0f : -0.0f;
    }
    if (cls == DUP_SAME_R || cls == MIXED) {  // the same value at the same r in two (or three) sub-tiles: equal keys
        const int r = pick_r(), n = 2 + (int)(rng() % 2u);
        const float val = low * (1.0f + uni(rng));
        for (int i = 0; i < n; ++i) at(pick_u(), r) = val;
        if (rng() & 1) at(pick_u(), pick_r()) = val * (1.0f + 0.5f * uni(rng));  // and sometimes a lower value after / before
    }
    if (cls == DUP_IN_SUBTILE || cls == MIXED) {  // the same value at several r of one sub-tile: keys differ by the tags
        const int u = pick_u(), n = 2 + (int)(rng() % 3u);
        const float val = low * (2.0f + uni(rng));
        for (int i = 0; i < n; ++i) at(u, pick_r()) = val;
    }
    if (cls == TRIPLES) {  // three equal values, lowest of the stream: same r three times, or spread
        const float val = low * 3.0f;
        const int r = pick_r();
        const bool same_r = rng() & 1;
        for (int i = 0; i < 3; ++i) at(pick_u(), same_r ? r : pick_r()) = val;
    }
    if (cls == PADDING || cls == MIXED) {
        npad = 1 + (int)(rng() % 15u);
        // codes beyond K are the highest of the last sub-tile, and a lane's codes ascend with r
        for (int i = 0; i < npad; ++i) at(nsub - 1, 15 - i) = INFINITY;
    }
}

static void run_stream(int cls, std::mt19937 &rng) {
    const int nsub = 32 + (int)(rng() % 65u), h = (int)(rng() & 1u);
    std::vector<float> v;
    int npad;
    make_stream(cls, rng, nsub, v, npad);
    ScrTrack t = scr_track_start();
    std::vector<KeyCode> all;
    for (int u = 0; u < nsub; ++u) {
        float acc[16];
        for (int r = 0; r < 16; ++r) {
            acc[r] = v[(size_t)u * 16 + r];
            if (u + 1 == nsub) acc[r] = scr_start_clamp(acc[r]);  // the kernel: start values of the last sub-tile
        }
        float key[16];
        std::memcpy(key, acc, sizeof key);
        scr_track_update(t, key, u);
        for (int r = 0; r < 16; ++r) {
            const float k = key[r];
            CHECK(bits(k) == bits(scr_tag(acc[r], r)), "%s: update left key %08x for value %08x r %d", kNames[cls], bits(k), bits(acc[r]), r);
            CHECK(k == k, "%s: NaN key from value %08x r %d", kNames[cls], bits(acc[r]), r);
            CHECK(std::llabs(ordinal(k) - ordinal(acc[r])) <= 15 && std::signbit(k) == std::signbit(acc[r]), "%s: key %08x of value %08x",
                  kNames[cls], bits(k), bits(acc[r]));
            if (std::isinf(v[(size_t)u * 16 + r]))
                CHECK(std::isfinite(k) && k >= 0x1p+99f, "%s: padding key %g", kNames[cls], (double)k);
            const int code = 32 * u + 4 * h + (r & 3) + 8 * (r >> 2);
            CHECK(scr_key_code(k, u, h) == code, "%s: code %d decoded as %d", kNames[cls], code, scr_key_code(k, u, h));
            all.push_back({k, code});
        }
    }
    std::stable_sort(all.begin(), all.end(), [](const KeyCode &a, const KeyCode &b) { return a.key < b.key; });
    // the three lowest keys, as a multiset (ascending on both sides; -0 and +0 keys differ in r or compare equal)
    const float got[3] = {t.b1, t.b2, t.b3};
    CHECK(t.b1 <= t.b2 && t.b2 <= t.b3, "%s: not sorted", kNames[cls]);
    for (int j = 0; j < 3; ++j)
        CHECK(got[j] == all[j].key, "%s: lowest %d is %08x, the sort has %08x", kNames[cls], j, bits(got[j]), bits(all[j].key));
    const int c1 = scr_key_code(t.b1, t.u1, h), c2 = scr_key_code(t.b2, t.u2, h);
    if (t.b1 < t.b2) CHECK(c1 == all[0].code, "%s (I1): b1 decoded as %d, the lowest key is code %d", kNames[cls], c1, all[0].code);
    if (t.b2 < t.b3) {
        const int lo = std::min(all[0].code, all[1].code), hi = std::max(all[0].code, all[1].code);
        CHECK(c1 != c2 && std::min(c1, c2) == lo && std::max(c1, c2) == hi, "%s (I2): decoded %d, %d, the two lowest keys are codes %d, %d",
              kNames[cls], c1, c2, all[0].code, all[1].code);
    }
    CHECK(t.u1 >= 0 && t.u1 < nsub && t.u2 >= 0 && t.u2 < nsub, "%s: sub-tiles %d, %d of %d", kNames[cls], t.u1, t.u2, nsub);
}

int main() {
    // the tag by itself: monotone for one r over neighbouring floats of both signs, zeros and subnormals included
    {
        std::mt19937 rng(1);
        for (int i = 0; i < 200000; ++i) {
            uint32_t b = rng();
            if ((b & 0x7F800000u) == 0x7F800000u) b &= 0xBFFFFFFFu;  // finite
            if (i % 7 == 0) b &= 0x800000FFu;                        // around zero
            const float a = from_bits(b);
            const float c = std::nextafter(a, INFINITY);
            if (!std::isfinite(c)) continue;
            for (int r = 0; r < 16; ++r) {
                const float ka = scr_tag(a, r), kc = scr_tag(c, r);
                CHECK(ka <= kc, "tag not monotone: %08x -> %08x, %08x -> %08x (r %d)", bits(a), bits(ka), bits(c), bits(kc), r);
                CHECK((bits(ka) & 15u) == (unsigned)r, "tag lost: %08x r %d", bits(ka), r);
            }
        }
        CHECK(bits(scr_tag(0.0f, 5)) == 5u && bits(scr_tag(-0.0f, 5)) == 0x80000005u, "zero keys");
        CHECK(scr_start_clamp(INFINITY) == kScrPadStart && scr_start_clamp(NAN) == kScrPadStart && scr_start_clamp(0x1p+29f) == 0x1p+29f &&
                  scr_start_clamp(-1.0f) == -1.0f,
              "start clamp");
    }
    for (int cls = 0; cls < NCLASS; ++cls) {
        std::mt19937 rng(100 + cls);
        for (int i = 0; i < 1000; ++i) run_stream(cls, rng);
    }
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("scr keys ok\n");
    return 0;
}
