// vq_scr_keys.h -- what a lane of the screened Dp = 256 sweep keeps of its codes (vq_search_persist<.., SCREEN>,
// vq_search_persist.inc): the three lowest screened values and WHICH codes the two lowest belong to, without ever searching
// the accumulator registers for a value.  The same code on the host and on the device (the device runs the three-lowest
// block as inline assembly); a host program can include this file alone (tests/cabi/scr_keys.cpp).
//
// A sub-tile u leaves a lane 16 accumulator values v[0..15], v[r] the value of code 32 u + 4 h + (r & 3) + 8 (r >> 2) (h =
// the lane's half).  The position r goes INTO the value: the 4 low mantissa bits of v[r] are overwritten with r.  The result
// is the code's KEY; every comparison after that -- the three lowest, the certainty test, the candidate thresholds -- is made
// on keys, so the bound of vq_search_persist.inc carries the perturbation (item (6) there):
//  * |key - v| <= 15 ulp(v) <= 15 * 2^-23 |v| for a normal v, <= 15 * 2^-149 below 2^-126;
//  * for one r the map v -> key is monotone (non-decreasing) over all floats of both signs: the bit pattern's upper 28 bits
//    order the magnitudes, and floats that share them share the key;
//  * two codes of one lane and one sub-tile never have equal keys (their r differ); equal keys mean the same r in two
//    sub-tiles.  Among equal VALUES of one sub-tile the lower r, which is the lower code, has the lower key.
//  * +inf would become a NaN for r != 0, and v_med3_f32 answers min3 when an operand is a NaN.  The one source of +inf in a
//    sweep of finite rows is the |c|^2 s_c s_x of the padding codes behind K, so the sweep starts the LAST sub-tile's
//    accumulators from min(that, kScrPadStart) (scr_start_clamp).  Real codes are not touched: s_c and s_x put their
//    |c|^2 s_c s_x below 256 * 2^13 * 2^8 = 2^29.  A padding code's accumulator is kScrPadStart plus products of at most
//    2^38 in all, its key is finite and >= 2^99, and a threshold of an eligible row (b1 + 2 delta + w, in the accumulator's
//    units below 2^36: |c|^2 term 2^29, dot products 2^18 * 2^15 = 2^33) never reaches it.  Rows that are not finite make NaN
//    keys whatever the start; they are ineligible, searched again in full, and only need a provisional code below K.
//
// The tracker.  b1 <= b2 <= b3 are the three lowest keys so far (a multiset: equal keys count as often as they occur), u1 and
// u2 the sub-tiles in which b1 and b2 arrived.  One sub-tile: b3 = med3(b2, b3, k), b2 = med3(b1, b2, k), b1 = min(b1, k) for
// each of the 16 keys k (each med3 is the new j-th lowest because b1 <= b2 <= b3), then
//  * b1 fell            -> u1 = u;
//  * b2 fell            -> u2 = the old u1 if b1 fell and b2 is the old b1 (the old lowest, demoted), else u.
// The code of a key is recovered from (key & 15, its sub-tile, h) once, after the sweep (scr_key_code).
// What the certainty test and the rescore list need, and what holds (tests/cabi/scr_keys.cpp checks both against a sort):
//  (I1) b1 < b2            => scr_key_code(b1, u1, h) is the code of the lane's lowest key;
//  (I2) b2 < b3            => {scr_key_code(b1, u1, h), scr_key_code(b2, u2, h)} are the codes of the lane's two lowest keys
//       (two different codes, also when b1 == b2: the same r in two sub-tiles -- u1 keeps the earlier one, because b1 falls
//       only on a strictly lower key, and u2 takes the later one).
// Hence for a threshold thr < b3 the decoded codes of all keys <= thr are right.  When b2 == b3 the attribution of b2 may be
// that of another code with the same key (a demoted b1 and a new key equal to it cannot be told apart); such a lane has
// b3 <= thr whenever b2 <= thr, the row is then not `complete` and is searched again in full.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VQ_KEYS_FN __host__ __device__ __forceinline__
#else
#define VQ_KEYS_FN inline
#endif

constexpr float kScrPadStart = 0x1p+100f;  // start value of a padding code's accumulator (see above)

struct ScrTrack {
    float b1, b2, b3;  // the three lowest keys, b1 <= b2 <= b3
    int u1, u2;        // sub-tiles of b1 and b2
};

VQ_KEYS_FN unsigned scr_float_bits(float v) { return __builtin_bit_cast(unsigned, v); }
VQ_KEYS_FN float scr_bits_float(unsigned b) { return __builtin_bit_cast(float, b); }

// the key of accumulator register r holding v
VQ_KEYS_FN float scr_tag(float v, int r) { return scr_bits_float((scr_float_bits(v) & ~15u) | (unsigned)r); }
// the start value of an accumulator of the last sub-tile (never a NaN, never above kScrPadStart)
VQ_KEYS_FN float scr_start_clamp(float cn_scaled) { return cn_scaled < kScrPadStart ? cn_scaled : kScrPadStart; }
// the code a key of sub-tile u belongs to, in lane half h (the accumulator layout of run_sub_scr)
VQ_KEYS_FN int scr_key_code(float key, int u, int h) {
    const int r = (int)(scr_float_bits(key) & 15u);
    return 32 * u + 4 * h + (r & 3) + 8 * (r >> 2);
}

VQ_KEYS_FN ScrTrack scr_track_start() {
    ScrTrack t;
    t.b1 = t.b2 = t.b3 = __builtin_inff();
    t.u1 = t.u2 = 0;
    return t;
}

// v_med3_f32 and v_min_f32 as the host sees them (no NaN reaches them from finite rows)
VQ_KEYS_FN float scr_min(float a, float b) { return b < a ? b : a; }
VQ_KEYS_FN float scr_med3(float a, float b, float c) {
    const float lo = scr_min(a, b), hi = b < a ? a : b;
    return c < lo ? lo : (hi < c ? hi : c);
}

// One sub-tile: v[0..15] (an f32x16 or an array) are replaced by their keys and folded into t.
template <class V>
VQ_KEYS_FN void scr_track_update(ScrTrack &t, V &v, int u) {
    const float o1 = t.b1, o2 = t.b2;
#if defined(__HIP_DEVICE_COMPILE__)
    // 16 x (tag in place, b3, b2, b1): 64 VALU instructions, no branch
#define VQ_SCR_STEP(n, r)                                                                                                   \
    "v_bfi_b32 %" #n ", 15, " #r ", %" #n "\n\tv_med3_f32 %2, %1, %2, %" #n "\n\tv_med3_f32 %1, %0, %1, %" #n "\n\tv_min_f32 %0, %0, %" \
    #n "\n\t"
    asm(VQ_SCR_STEP(3, 0) VQ_SCR_STEP(4, 1) VQ_SCR_STEP(5, 2) VQ_SCR_STEP(6, 3) VQ_SCR_STEP(7, 4) VQ_SCR_STEP(8, 5) VQ_SCR_STEP(9, 6)
        VQ_SCR_STEP(10, 7) VQ_SCR_STEP(11, 8) VQ_SCR_STEP(12, 9) VQ_SCR_STEP(13, 10) VQ_SCR_STEP(14, 11) VQ_SCR_STEP(15, 12)
        VQ_SCR_STEP(16, 13) VQ_SCR_STEP(17, 14) VQ_SCR_STEP(18, 15)
        : "+v"(t.b1), "+v"(t.b2), "+v"(t.b3), "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]),
          "+v"(v[7]), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]));
#undef VQ_SCR_STEP
#else
    for (int r = 0; r < 16; ++r) {
        const float k = scr_tag(v[r], r);
        v[r] = k;
        t.b3 = scr_med3(t.b2, t.b3, k);
        t.b2 = scr_med3(t.b1, t.b2, k);
        t.b1 = scr_min(t.b1, k);
    }
#endif
    const bool nb1 = t.b1 < o1;
    const int ou1 = t.u1;
    t.u2 = (t.b2 < o2) ? ((nb1 && t.b2 == o1) ? ou1 : u) : t.u2;
    t.u1 = nb1 ? u : ou1;
}
