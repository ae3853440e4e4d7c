// The host side of a scene (csrc/trc_scene_host.h) without a device: the one validation of a caller's Kd-tree on a hand-made tree and
// on the malformed ones that used to reach the host's indexing, its packing, the layout of the tally buffer against sums written
// out, and the build order of the search tables.  Built with the address and undefined-behaviour sanitizers (make scenecheck), run
// by tests/test_scene_host.py.  The arrays of the malformed trees are exactly as long as their counts say: a read past them is found.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../tracer_amd/csrc/trc_scene_host.h"

static int bad = 0, checks = 0;
#define EXPECT(cond, ...) do { ++checks; if (!(cond)) { ++bad; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a tree of five nodes on three levels over four surfaces: 0 -> (1, 2), 1 -> (3, 4); leaves 2, 3, 4
struct Tree {
    std::vector<int32_t> flag{0, 1, 3, 3, 3}, child{1, 3, 0, 0, 0}, leaf_off{0, 0, 0, 2, 3}, leaf_cnt{0, 0, 2, 1, 2}, leaf_surfs{0, 1, 2, 1, 3}, always{2};
    std::vector<double> split{0.5, -0.25, 0.0, 0.0, 0.0};
    trc_kdtree_desc desc() const {
        trc_kdtree_desc kd;
        std::memset(&kd, 0, sizeof(kd));
        kd.n_nodes = (int32_t)flag.size(); kd.n_leaf_surfs = (int32_t)leaf_surfs.size(); kd.n_always = (int32_t)always.size();
        kd.flag = flag.data(); kd.split = split.data(); kd.child = child.data(); kd.leaf_off = leaf_off.data(); kd.leaf_cnt = leaf_cnt.data();
        kd.leaf_surfs = leaf_surfs.data(); kd.always_relevant = always.data();
        const double b[6] = {-1, -1, -1, 1, 1, 1};
        std::memcpy(kd.bounds, b, sizeof(b));
        return kd;
    }
};

static void refused(const char *what, const trc_kdtree_desc &kd, int n_surf) {
    char msg[256] = "";
    int depth = -1;
    const int st = trc_kd_check(&kd, n_surf, &depth, msg, sizeof(msg));
    EXPECT(st == TRC_ERR_INVALID && msg[0] != 0, "%s: status %d, message '%s'", what, st, msg);
}

struct MapSize { int nu, nv; };

static trc_surface_desc rect_at(double x, double y, double z) {
    trc_surface_desc s;
    std::memset(&s, 0, sizeof(s));
    s.gm_kind = TRC_GM_RECT; s.optics_kind = 0; s.extra_off = -1;
    s.frame[0] = s.frame[5] = s.frame[10] = 1.0;
    s.frame[3] = x; s.frame[7] = y; s.frame[11] = z;
    s.gm[0] = 1.0; s.gm[1] = 0.5;
    return s;
}

int main() {
    const Tree good;
    char msg[256] = "";
    {   // accepted, with its depth, and packed
        const trc_kdtree_desc kd = good.desc();
        int depth = -1;
        const int st = trc_kd_check(&kd, 4, &depth, msg, sizeof(msg));
        EXPECT(st == TRC_OK && depth == 2, "status %d, depth %d, '%s'", st, depth, msg);
        std::vector<int32_t> a, b;
        trc_kd_pack(&kd, a, b);
        const std::vector<int32_t> a_want{(1 << 2) | 0, (3 << 2) | 1, (0 << 2) | 3, (2 << 2) | 3, (3 << 2) | 3}, b_want{0, 0, 2, 1, 2};
        EXPECT(a == a_want && b == b_want, "packed words differ");
    }
    {   // NULL leaf_surfs with a non-empty leaf
        trc_kdtree_desc kd = good.desc(); kd.leaf_surfs = nullptr;
        refused("NULL leaf_surfs", kd, 4);
    }
    {   // NULL always_relevant with n_always > 0
        trc_kdtree_desc kd = good.desc(); kd.always_relevant = nullptr;
        refused("NULL always_relevant", kd, 4);
    }
    {   // negative counts
        trc_kdtree_desc kd = good.desc(); kd.n_leaf_surfs = -1;
        refused("n_leaf_surfs < 0", kd, 4);
        kd = good.desc(); kd.n_always = -3;
        refused("n_always < 0", kd, 4);
        kd = good.desc(); kd.n_nodes = -5;
        refused("n_nodes < 0", kd, 4);
        kd = good.desc(); kd.n_nodes = 0;
        refused("n_nodes == 0", kd, 4);
    }
    {   // a leaf range whose end wraps in 32 bits
        Tree t; t.leaf_off[4] = INT32_MAX; t.leaf_cnt[4] = 1;
        refused("leaf_off INT32_MAX + 1", t.desc(), 4);
        Tree u; u.leaf_cnt[2] = 6;
        refused("leaf range past leaf_surfs", u.desc(), 4);
    }
    {   // a child not behind its parent, and one whose sibling is past the end
        Tree t; t.child[1] = 1;
        refused("child == parent", t.desc(), 4);
        Tree u; u.child[1] = 0;
        refused("child before parent", u.desc(), 4);
        Tree v; v.child[1] = 4;
        refused("sibling past the end", v.desc(), 4);
    }
    {   // a flag of 4
        Tree t; t.flag[2] = 4;
        refused("flag 4", t.desc(), 4);
        Tree u; u.flag[0] = -1;
        refused("flag -1", u.desc(), 4);
    }
    {   // a surface index equal to n_surf, in a leaf, in an entry no leaf names, and among the always relevant
        refused("leaf surface == n_surf", good.desc(), 3);
        Tree t; t.leaf_surfs.push_back(4);
        refused("unnamed leaf entry == n_surf", t.desc(), 4);
        Tree u; u.always[0] = 4;
        refused("always-relevant == n_surf", u.desc(), 4);
        Tree v; v.leaf_surfs[0] = -1;
        refused("leaf surface -1", v.desc(), 4);
    }
    {   // the tally buffer of seven surfaces with a 3 x 5 and a 1 x 1 map: 3 * 7 + 2 = 23 | 15 | 1 | 8 * 7 = 56
        const MapSize maps[2] = {{3, 5}, {1, 1}};
        const trc_tally_plan off = trc_tally_layout(7, maps, 2, false), on = trc_tally_layout(7, maps, 2, true);
        EXPECT(off.bins.size() == 2 && off.bins[0] == 23 && off.bins[1] == 38, "bins off");
        EXPECT(on.bins == off.bins, "bins move when the matrix is toggled");
        EXPECT(off.tr_off == -1 && off.total == 39, "off: %lld %lld", (long long)off.tr_off, (long long)off.total);
        EXPECT(on.tr_off == 23 + 15 + 1 && on.total == 23 + 15 + 1 + 56, "on: %lld %lld", (long long)on.tr_off, (long long)on.total);   // (39 doubles before the matrix: it starts at 39, 95 in all)
        const trc_tally_plan one = trc_tally_layout(1, (const MapSize *)nullptr, 0, false);
        EXPECT(one.bins.empty() && one.tr_off == -1 && one.total == 5, "one surface: %lld", (long long)one.total);
    }
    {   // the search tables of twelve rectangles: the LDS-sized grid, and the large one when the small one is forced off
        std::vector<trc_surface_desc> s;
        for (int i = 0; i < 12; ++i) s.push_back(rect_at(2.0 * (i % 4), 1.5 * (i / 4), 0.1 * i));
        trc_accel_host A{}, B{};
        trc_search_tables_build(s.data(), 12, false, A);
        EXPECT(A.grid_ok && !A.big_ok, "plain: grid_ok %d big_ok %d", (int)A.grid_ok, (int)A.big_ok);
        trc_search_tables_build(s.data(), 12, true, B);
        EXPECT(!B.grid_ok && B.big_ok, "force32: grid_ok %d big_ok %d", (int)B.grid_ok, (int)B.big_ok);
        EXPECT(A.sbox == B.sbox && A.brute_leaf == B.brute_leaf && A.sbox.size() == 72, "boxes differ");
        EXPECT(trc_scene_stride(s.data(), 12) == ((TRC_REC_HDR + trc_gm_nparams(TRC_GM_RECT)) | 1), "stride");
        bool splits = true;
        CarryNeeds needs;
        trc_scene_scan(s.data(), 12, &splits, &needs);
        EXPECT(!splits && !needs.any(), "scan of plain mirrors");
        s[5].optics_kind = TRC_OPT_REFRACTIVE_MATERIAL; s[5].opt[0] = 0.0; s[5].opt[4] = 2; s[5].opt[5] = 7;
        s[9].optics_kind = TRC_OPT_LAMBERTIAN_POLYCHROMATIC;
        trc_scene_scan(s.data(), 12, &splits, &needs);
        EXPECT(splits && needs.max_mat == 7 && needs.poly, "scan: %d %d %d", (int)splits, needs.max_mat, (int)needs.poly);
    }
    std::printf("%d checks, %d violations\n", checks, bad);
    return bad > 255 ? 255 : bad;
}
