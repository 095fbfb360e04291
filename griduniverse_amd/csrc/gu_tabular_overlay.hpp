// gu_tabular_overlay.hpp -- the five overlay kinds as the learners' lane knows them (gu_tabular.hpp: TabLane's OV and NoOverlay, which
// lists what a kind supplies; gu_td.hip and gu_eval.hip include this).  Each struct holds its kind's fields and states its rule once, on the
// device helpers of gu_map.hpp that the kind's own step and rollout kernels use.  move() is TabLane::move's whole rule under the kind:
// from cell l.s of the lane `l` with action ua it sets l.r, l.d and the word behind the move and returns s' (l.wd: the kind's plane,
// l.prefix and l.t: the lane's stream prefix and step count).  It starts from gu_move's candidate itself, and reads the lane through
// `l`, because that is the form the compiler turns into the code these rules had inside TabLane (profiles/learner_overlay_asm.txt).
#pragma once
#include "gu_tabular.hpp"

// Wind (include/gu.h: gu_set_wind; GUST: the engine has a gust probability): move() pushes the agent behind its action, with the wind
// of the cell it leaves, gusting on the stream-9 word of step t (hashed only where some lane of the wave stands in wind).
template <bool GUST>
struct WindOverlay : NoOverlay {
    static constexpr int PLANES = 3;
    uint32_t gust_q16;  // GUST: the engine's gust probability
    __device__ __forceinline__ void load(const OverlayLaneArgs &o, int64_t) { gust_q16 = o.param; }
    template <bool LDS, class L>
    __device__ __forceinline__ int32_t move(L &l, const TabArgs &a, uint32_t ua)
    {
        int32_t s2 = gu_move(l.s, l.m.f[l.s], ua, gu_delta<LDS>(ua, a.lut, a.W));
        const uint32_t c = l.wd[l.s];
        uint32_t k = GU_WIND_STRENGTH(c);
        if (GUST && __builtin_amdgcn_ballot_w64(k > 0u) != 0ull) k = gu_wind_gust(k, gu_rng_word(l.prefix, GU_RNG_STREAM_WIND, (uint32_t)l.t), gust_q16);
        s2 = gu_wind_push<LDS>(l.m.f, s2, c, k, a.lut, a.W);
        l.r = l.m.r[s2];
        l.d = (l.m.f[s2] >> GU_CELL_TERM_BIT) & 1;
        return s2;
    }
};

// Fruit (gu_set_fruit): the table has S << F rows and the lane stands on row eaten * S + s.  A wall bump onto an uneaten fruit keeps the
// cell and changes the row.  The fruit byte of s' is read beside its flags and its reward byte: the chain does not grow.
struct FruitOverlay {
    static constexpr int PLANES = 3;
    static constexpr bool MASKED = true;
    uint32_t values, eaten, eaten2;  // the kinds' values; the env's mask of eaten fruit, and the one behind move()
    __device__ __forceinline__ void load(const OverlayLaneArgs &o, int64_t e) { values = o.param, eaten = o.word[e]; }
    __device__ __forceinline__ void begin(const uint8_t *) { eaten2 = eaten; }
    __device__ __forceinline__ void reset(uint32_t, uint32_t) { eaten = eaten2 = 0u; }  // the fruit grows back
    template <bool LDS, class L>
    __device__ __forceinline__ int32_t move(L &l, const TabArgs &a, uint32_t ua)
    {
        const int32_t s2 = gu_move(l.s, l.m.f[l.s], ua, gu_delta<LDS>(ua, a.lut, a.W));
        l.r = l.m.r[s2];
        l.r += gu_fruit_eat(l.wd[s2], values, eaten2);
        l.d = (l.m.f[s2] >> GU_CELL_TERM_BIT) & 1;
        return s2;
    }
    __device__ __forceinline__ void commit() { eaten = eaten2; }
    __device__ __forceinline__ uint32_t key() const { return eaten; }
    __device__ __forceinline__ uint32_t key2() const { return eaten2; }
    __device__ __forceinline__ void store(const OverlayLaneArgs &o, int64_t e) const { o.word[e] = eaten; }
};

// Doors (gu_set_doors): the table has S << D rows and the lane stands on row open * S + s.  A closed door refuses entry as a wall does;
// the key or lever of a cell ENTERED changes the mask behind the step.  The door byte of the candidate is read BESIDE its flags and
// reward byte, and the gate picks between them and the bytes of s, read beside each other (the head of gu_doors.hip carries them
// instead): two rounds of reads on the chain, as without doors.
struct DoorOverlay {
    static constexpr int PLANES = 3;
    static constexpr bool MASKED = true;
    uint32_t open, open2;  // the env's mask of open slots, and the one behind move()
    __device__ __forceinline__ void load(const OverlayLaneArgs &o, int64_t e) { open = o.word[e]; }
    __device__ __forceinline__ void begin(const uint8_t *) { open2 = open; }
    __device__ __forceinline__ void reset(uint32_t, uint32_t) { open = open2 = 0u; }  // the doors are shut again
    template <bool LDS, class L>
    __device__ __forceinline__ int32_t move(L &l, const TabArgs &a, uint32_t ua)
    {
        int32_t s2 = gu_move(l.s, l.m.f[l.s], ua, gu_delta<LDS>(ua, a.lut, a.W));
        const uint32_t c = l.wd[s2];
        const bool shut = gu_door_closed(c, open);
        open2 = gu_door_touch(c, open, !shut && s2 != l.s);
        l.r = shut ? l.m.r[l.s] : l.m.r[s2];
        l.d = ((shut ? l.m.f[l.s] : l.m.f[s2]) >> GU_CELL_TERM_BIT) & 1;
        return shut ? l.s : s2;
    }
    __device__ __forceinline__ void commit() { open = open2; }
    __device__ __forceinline__ uint32_t key() const { return open; }
    __device__ __forceinline__ uint32_t key2() const { return open2; }
    __device__ __forceinline__ void store(const OverlayLaneArgs &o, int64_t e) const { o.word[e] = open; }
};

// Boxes (gu_set_boxes): the table has S << (b * B) rows and the lane stands on row word * S + s.  The lane carries the count of boxes
// on a target beside the word of box cells, as the rollout kernel does (the head of gu_boxes.hip); move() applies rules 2-6 of
// gu_set_boxes on the candidate (BoxRule::move of gu_boxes.hip, with the bytes of s' read behind the push), the push behind a branch
// that only pushing lanes take.
struct BoxOverlay {
    static constexpr int PLANES = 3;
    static constexpr bool MASKED = true;
    uint32_t param, init;  // GU_BOX_PARAM, and the word at reset
    uint32_t on, on2, word, word2;  // boxes on a target and the word of box cells, each with the one behind move()
    __device__ __forceinline__ void load(const OverlayLaneArgs &o, int64_t e) { param = o.param, init = o.init, word = o.word[e]; }
    __device__ __forceinline__ void begin(const uint8_t *wd) { word2 = word, on = on2 = gu_box_on_target(wd, word, GU_BOX_B(param), GU_BOX_BITS(param)); }
    __device__ __forceinline__ void reset(uint32_t, uint32_t) { word = word2 = init, on = on2 = GU_BOX_ON0(param); }  // the boxes are back where they began
    template <bool LDS, class L>
    __device__ __forceinline__ int32_t move(L &l, const TabArgs &a, uint32_t ua)
    {
        int32_t s2 = gu_move(l.s, l.m.f[l.s], ua, gu_delta<LDS>(ua, a.lut, a.W));
        const uint32_t B = GU_BOX_B(param), b = GU_BOX_BITS(param);
        const bool solved = on == B;
        const int32_t c = s2, at = gu_box_at(word, c, B, b), k = ((c != l.s) & !solved) ? at : -1;
        bool stay = solved;
        int32_t gain = 0;
        word2 = word;
        if (k >= 0) stay = gu_box_push(l.m.f, l.wd, c, l.m.f[c], l.wd[c], ua, gu_delta<LDS>(ua, a.lut, a.W), k, B, b, word2, gain);
        s2 = stay ? l.s : c;
        on2 = on + (uint32_t)gain;
        const bool won = on2 == B;
        l.r = won ? GU_BOX_SOLVED_REWARD : l.m.r[s2] + GU_BOX_V(param) * gain;
        l.d = won ? 1 : (l.m.f[s2] >> GU_CELL_TERM_BIT) & 1;
        return s2;
    }
    __device__ __forceinline__ void commit() { word = word2, on = on2; }
    __device__ __forceinline__ uint32_t key() const { return word; }
    __device__ __forceinline__ uint32_t key2() const { return word2; }
    __device__ __forceinline__ void store(const OverlayLaneArgs &o, int64_t e) const { o.word[e] = word; }
};

// Errands (gu_set_errands): the plane has fruit's format, the table has S << (F + pb + ib) rows and the lane stands on row word * S + s,
// word = eaten | progress | instruction.  The lane carries `rem`, its instruction byte shifted right by 2p, beside the word, as the
// rollout kernel does (the head of gu_errands.hip); reset() draws the instruction on stream 11 at the episode count before the reset
// and move() applies rules 2-5 of gu_set_errands on the candidate, its three bytes read together; a completed word keeps the cell
// behind the reads.
struct ErrandOverlay {
    static constexpr int PLANES = 3;
    static constexpr bool MASKED = true;
    uint32_t instr, param2;  // the instructions, and GU_ERRAND_PARAM2
    uint32_t word, word2, rem, rem2;  // the env's word and the rest of its instruction, and the two behind move()
    __device__ __forceinline__ void load(const OverlayLaneArgs &o, int64_t e) { instr = o.param, param2 = o.param2, word = o.word[e]; }
    __device__ __forceinline__ void begin(const uint8_t *) { word2 = word, rem = rem2 = gu_errand_rem(word, instr, param2); }
    __device__ __forceinline__ void reset(uint32_t start_prefix, uint32_t ep)
    {
        gu_errand_draw(start_prefix, ep, instr, param2, word, rem);
        word2 = word, rem2 = rem;
    }
    template <bool LDS, class L>
    __device__ __forceinline__ int32_t move(L &l, const TabArgs &a, uint32_t ua)
    {
        const int32_t s2 = gu_move(l.s, l.m.f[l.s], ua, gu_delta<LDS>(ua, a.lut, a.W));
        word2 = word, rem2 = rem;
        const bool stay = gu_errand_touch(l.wd[s2], l.m.r[s2], (l.m.f[s2] >> GU_CELL_TERM_BIT) & 1, param2, word2, rem2, l.r, l.d);
        return stay ? l.s : s2;
    }
    __device__ __forceinline__ void commit() { word = word2, rem = rem2; }
    __device__ __forceinline__ uint32_t key() const { return word; }
    __device__ __forceinline__ uint32_t key2() const { return word2; }
    __device__ __forceinline__ void store(const OverlayLaneArgs &o, int64_t e) const { o.word[e] = word; }
};
