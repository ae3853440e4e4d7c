// The room of a streaming call whose optics split rays (trc_split_room_need, trc_split_grow: csrc/trc_bounds.h), as the host
// driver uses them before every bounce, checked on a grid of inputs.  A program of its own (`make splitcheck` builds it with
// -fsanitize=address,undefined; tests/test_split_cases_host.py runs it): prints one line per violated property and returns their
// number.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../tracer_amd/csrc/trc_core.h"
#include "../../tracer_amd/csrc/trc_bounds.h"

static int bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; if (bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
    const trc_u64 MAXU = ~0ull;
    // values around what a call meets, the 32-bit and 64-bit borders included
    const std::vector<trc_u64> counts = {0, 1, 63, 64, 65, 200, 256, 2048, 19914, 1ull << 20, (1ull << 26) + 37, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1, 1ull << 32};
    const std::vector<trc_u64> waves = {0, 1, 16, 4096, 5120, 16384};
    const std::vector<trc_u64> chunks = {64, 128, 256, 1024};
    long long n = 0;
    for (trc_u64 slots : counts) for (trc_u64 live : counts) for (trc_u64 sw : waves) for (trc_u64 w : waves) for (trc_u64 sc : chunks) for (trc_u64 ac : chunks) {
        const trc_u64 tails = sw * 256;
        const trc_split_room r = trc_split_room_need(slots, live, tails, w, sc, ac);
        ++n;
        // the ray table: every slot handed out, one new slot per live ray, one chunk unused per wave; the lists: every live ray and the tails
        EXPECT(r.room >= slots + live + w * sc, "slots %llu live %llu waves %llu chunk %llu: room %llu", slots, live, w, sc, r.room);
        EXPECT(r.room >= live + tails, "live %llu tails %llu: room %llu", live, tails, r.room);
        EXPECT(r.act_room >= 2 * live + w * ac, "live %llu waves %llu chunk %llu: act_room %llu", live, w, ac, r.act_room);
        // monotone in every argument
        const trc_split_room a = trc_split_room_need(slots + 1, live, tails, w, sc, ac), b = trc_split_room_need(slots, live + 1, tails, w, sc, ac),
                             c = trc_split_room_need(slots, live, tails + 64, w, sc, ac), d = trc_split_room_need(slots, live, tails, w + 1, sc, ac),
                             e = trc_split_room_need(slots, live, tails, w, sc + 64, ac), f = trc_split_room_need(slots, live, tails, w, sc, ac + 64);
        for (const trc_split_room &m : {a, b, c, d, e, f}) EXPECT(m.room >= r.room && m.act_room >= r.act_room, "not monotone at slots %llu live %llu", slots, live);
        // doubling reaches the need, keeps a table that is large enough, and at least doubles one that is not
        for (trc_u64 have : {0ull, 64ull, 2048ull, 1ull << 24, (1ull << 32) + 5}) {
            const trc_u64 g = trc_split_grow(have, r.room);
            EXPECT(g >= r.room && g >= have, "have %llu need %llu: %llu", have, r.room, g);
            if (r.room <= have) EXPECT(g == have, "have %llu need %llu: %llu", have, r.room, g);
            else EXPECT(g >= 2 * have && (have < 64 || g / have * have == g), "have %llu need %llu: %llu", have, r.room, g);
            if (r.room > 64 && r.room > have && have >= 64) EXPECT(g / 2 < r.room, "have %llu need %llu: %llu doubles once too often", have, r.room, g);
        }
    }
    // bounce 0: every ray of the batch may hit and split -- one slot from the search stage and one from the shading kernel each
    for (trc_u64 nb : counts) for (trc_u64 tails : {0ull, 1024ull, 1ull << 22}) for (trc_u64 w : waves) for (trc_u64 sc : chunks) {
        const trc_u64 slots0 = trc_split_slots_bounce0(nb, tails);
        EXPECT(slots0 >= nb + tails, "nb %llu tails %llu: %llu", nb, tails, slots0);
        const trc_split_room r = trc_split_room_need(slots0, nb, tails, w, sc, sc);
        EXPECT(r.room >= 2 * nb + tails + w * sc, "bounce 0, nb %llu tails %llu waves %llu chunk %llu: room %llu", nb, tails, w, sc, r.room);
    }
    EXPECT(trc_split_slots_bounce0(MAXU, 5) == MAXU, "trc_split_slots_bounce0 wrapped");
    // nothing wraps past 64 bits: the sums saturate, and doubling stops at the largest value
    EXPECT(trc_sat_add(MAXU, 1) == MAXU && trc_sat_add(MAXU - 1, 1) == MAXU && trc_sat_add(1, MAXU) == MAXU && trc_sat_add(3, 4) == 7, "trc_sat_add");
    EXPECT(trc_sat_mul(1ull << 32, 1ull << 32) == MAXU && trc_sat_mul(1ull << 32, (1ull << 32) - 1) == ((1ull << 32) - 1) << 32 && trc_sat_mul(0, MAXU) == 0 && trc_sat_mul(MAXU, 0) == 0, "trc_sat_mul");
    for (trc_u64 live : {1ull << 32, MAXU / 2, MAXU - 1, MAXU}) {
        const trc_split_room r = trc_split_room_need(MAXU - 5, live, MAXU / 3, 1ull << 40, 1ull << 30, 1ull << 30);
        EXPECT(r.room == MAXU && r.act_room == MAXU, "live %llu: %llu %llu", live, r.room, r.act_room);
        const trc_split_room q = trc_split_room_need(live, live, 0, 16384, 1024, 1024);
        EXPECT(q.room >= live && q.act_room >= live, "live %llu: %llu %llu wrapped", live, q.room, q.act_room);
    }
    for (trc_u64 have : {1ull, 64ull, (1ull << 63) - 1, 1ull << 63, MAXU - 1}) {
        EXPECT(trc_split_grow(have, MAXU) == MAXU, "have %llu", have);
        EXPECT(trc_split_grow(have, (1ull << 63) + 1) > (1ull << 63), "have %llu", have);
    }
    // 2^32 live rays: the need is exact, and what it grows to is a power-of-two multiple of what there was
    {
        const trc_split_room r = trc_split_room_need(1ull << 32, 1ull << 32, 0, 5120, 1024, 1024);
        EXPECT(r.room == (1ull << 33) + 5120ull * 1024 && r.act_room == (1ull << 33) + 5120ull * 1024, "%llu %llu", r.room, r.act_room);
        EXPECT(trc_split_grow(2048, r.room) == 2048ull << 23, "%llu", trc_split_grow(2048, r.room));
    }
    std::printf("%lld combinations, %d violations\n", n, bad);
    return bad > 255 ? 255 : bad;
}
