// trc_mega.inc -- the two kernels of the persistent megakernel, as text that trc_kernels.hip includes twice: once as k_trace_fast /
// k_trace_coop<THREADS, SPEC, SUN, CHART>, the instances there have always been, and once as k_lamp_fast / k_lamp_coop<THREADS, SPEC,
// CHART> for the arc-lamp sources (trc_lamp_ray_t).  Text, and not a body that both kernels call: inlined from a function of its
// own the same body compiled to other scalar-register spills in every existing instance (`make asm`), and a template argument more
// would have renamed them all.  The including file defines MEGA_KERNEL_FAST and MEGA_KERNEL_COOP (the kernels' heads, with the
// parameter FastParams P), MEGA_SUN and MEGA_LAMP (fast_new_ray's SUN and LAMP).

// Generic fast kernel: float64 Kd traversal / brute force straight from trc_core.h; scene records (+ Kd arrays)
// staged in LDS when they fit in 64 KiB, read from global memory otherwise.  Used when the single-precision data
// cannot be built or do not fit (very large scenes), and as a cross-check of the cooperative kernel.
//   LDS (doubles): [recs S*stride][kd_split nodes][buie 639][tally 3S+2] then int32: [kd_a][kd_b][leaf][always]
MEGA_KERNEL_FAST {
    extern __shared__ double lds[];
    const DScene &sc = P.sc;
    const int S = sc.n_surf;
    const int tid = threadIdx.x;
    const unsigned lane = lane_id();

    const double *recs = sc.recs;
    const double *kd_split = sc.kd_split;
    const int32_t *kd_a = sc.kd_a, *kd_b = sc.kd_b, *kd_leaf = sc.kd_leaf, *kd_always = sc.kd_always;
    double *cursor = lds;
    if (P.lds_scene) {
        double *l_recs = cursor; cursor += (size_t)S * sc.stride;
        for (int i = tid; i < S * sc.stride; i += THREADS) l_recs[i] = sc.recs[i];
        recs = l_recs;
        if (sc.has_kd) {
            double *l_split = cursor; cursor += sc.kd_nodes;
            for (int i = tid; i < sc.kd_nodes; i += THREADS) l_split[i] = sc.kd_split[i];
            kd_split = l_split;
        }
    }
    const double *buie = nullptr;
    if (P.src) {
        const int NB = TRC_BUIE_TABLE;
        double *l_buie = cursor; cursor += TRC_BUIE_STAGED;
        if (P.src->kind == TRC_SRC_BUIE_DISK || P.src->kind == TRC_SRC_BUIE_RECT) {
            for (int i = tid; i < NB; i += THREADS) l_buie[i] = P.src->buie[i];
            if (tid == 0) trc_buie_aureole_consts(P.src->buie, l_buie + NB);
        }
        buie = l_buie;
    }
    double *l_tally = cursor;
    if (P.lds_tally) {
        cursor += 3 * S + 2;
        for (int i = tid; i < 3 * S + 2; i += THREADS) l_tally[i] = 0.0;
    }
    if (P.lds_scene && sc.has_kd) {
        int32_t *ic = (int32_t *)cursor;
        int32_t *l_a = ic; ic += sc.kd_nodes;
        int32_t *l_b = ic; ic += sc.kd_nodes;
        int32_t *l_leaf = ic; ic += sc.kd_nleaf;
        int32_t *l_alw = ic;
        for (int i = tid; i < sc.kd_nodes; i += THREADS) { l_a[i] = sc.kd_a[i]; l_b[i] = sc.kd_b[i]; }
        for (int i = tid; i < sc.kd_nleaf; i += THREADS) l_leaf[i] = sc.kd_leaf[i];
        for (int i = tid; i < sc.kd_nalways; i += THREADS) l_alw[i] = sc.kd_always[i];
        kd_a = l_a; kd_b = l_b; kd_leaf = l_leaf; kd_always = l_alw;
    }
    __syncthreads();

    const bool accel = sc.has_kd && (P.flags & TRC_TRACE_ACCEL);
    trc_kd_view kd = make_kd_view(sc, kd_a, kd_b, kd_split, kd_leaf, kd_always);

    // this wave's slice of the ray-id range
    const long long n_waves = (long long)gridDim.x * (THREADS >> 6);
    const long long wave = (long long)blockIdx.x * (THREADS >> 6) + (tid >> 6);
    const long long chunk = (P.n + n_waves - 1) / n_waves;
    long long next = wave * chunk;
    long long end = next + chunk;
    if (end > P.n) end = P.n;
    if (next > end) next = end;

    bool alive = false;
    double px = 0, py = 0, pz = 0, dx = 0, dy = 0, dz = 0, e = 0, ref = 1.0, wl = 0.0;
    unsigned long long rid = 0;
    int bounce = 0;
    int prev = S;              // surface the ray left (transfer matrix); S = the source
    double nseg = 0.0, nhit = 0.0;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    for (;;) {
        // ---- refill dead lanes with fresh rays (ballot + prefix rank) ----
        unsigned long long need = __ballot(!alive);
        if (next < end && need) {
            long long id = next + __popcll(need & lt_mask);
            if (!alive && id < end) {
                fast_new_ray<-1, SPEC, MEGA_SUN, MEGA_LAMP>(P, buie, id, px, py, pz, dx, dy, dz, e, ref, wl, rid);
                bounce = 0;
                prev = S;
                alive = true;
            }
            next += __popcll(need);
        }
        if (!__ballot(alive)) break;
        if (!alive) continue;

        // ---- one segment ----
        nseg += 1.0;
        double t;
        int s;
        if (accel) {
            LocalKdStack stk;
            trc_nearest_kd(kd, stk, recs, sc.stride, sc.extra, px, py, pz, dx, dy, dz, &t, &s);
        } else {
            trc_nearest_brute(recs, sc.stride, S, sc.extra, px, py, pz, dx, dy, dz, &t, &s);
        }
        if (s < 0) { alive = false; continue; }
        nhit += 1.0;
        if (P.lds_tally) alive = fast_shade<true, false, CHART>(P, recs, l_tally, t, s, px, py, pz, dx, dy, dz, e, ref, wl, rid, bounce, prev);
        else alive = fast_shade<false, false, CHART>(P, recs, l_tally, t, s, px, py, pz, dx, dy, dz, e, ref, wl, rid, bounce, prev);
    }

    // ---- flush ----
    nseg = wave_sum(nseg);
    nhit = wave_sum(nhit);
    if (P.lds_tally) {
        if (lane == 0) { atomicAdd(&l_tally[3 * S], nseg); atomicAdd(&l_tally[3 * S + 1], nhit); }
        __syncthreads();
        flush_sums<THREADS>(sc.tally, l_tally, 3 * S + 2, nullptr, 0, S);
    } else if (lane == 0) {
        atomicAdd(&sc.tally[3 * S], nseg);
        atomicAdd(&sc.tally[3 * S + 1], nhit);
    }
}

// Cooperative fast kernel (see the block comment above).  Exact tests read the surface records from global
// memory (they are rare); everything the candidate search touches lives in LDS:
//   doubles [buie 639][tally 3S+2] | float [sbox 6S] | u32 [nodes 2n] | i32 [always][unbounded] | u16 [leaf] |
//   16-byte aligned per-wave regions of COOP_WAVE_BYTES(depth)
MEGA_KERNEL_COOP {
    extern __shared__ double lds[];
    const DScene &sc = P.sc;
    const int S = sc.n_surf;
    const int tid = threadIdx.x;
    const unsigned lane = lane_id();
    const double *recs = sc.recs;

    double *cursor = lds;
    const double *buie = nullptr;
    if (P.src) {
        const int NB = TRC_BUIE_TABLE;
        double *l_buie = cursor; cursor += TRC_BUIE_STAGED;
        if (P.src->kind == TRC_SRC_BUIE_DISK || P.src->kind == TRC_SRC_BUIE_RECT) {
            for (int i = tid; i < NB; i += THREADS) l_buie[i] = P.src->buie[i];
            if (tid == 0) trc_buie_aureole_consts(P.src->buie, l_buie + NB);
        }
        buie = l_buie;
    }
    double *l_tally = cursor;
    cursor += 3 * S + 2;
    for (int i = tid; i < 3 * S + 2; i += THREADS) l_tally[i] = 0.0;

    const bool kd32 = sc.a_kd_ok && (P.flags & TRC_TRACE_ACCEL);
    trc_accel_view A;
    CoopLds W;
    {
        float *l_sbox = (float *)cursor;
        for (int i = tid; i < 6 * S; i += THREADS) l_sbox[i] = sc.a_sbox[i];
        uint32_t *l_nodes = (uint32_t *)(l_sbox + 6 * S);
        const int nn = kd32 ? sc.kd_nodes : 1;          // without a Kd-tree: one leaf holding every bounded surface
        for (int i = tid; i < 2 * nn; i += THREADS) l_nodes[i] = kd32 ? sc.a_nodes[i] : sc.a_bnodes[i];
        int32_t *l_alw = (int32_t *)(l_nodes + 2 * nn);
        const int na = kd32 ? sc.kd_nalways : 0;
        for (int i = tid; i < na; i += THREADS) l_alw[i] = sc.kd_always[i];
        int32_t *l_unb = l_alw + na;
        for (int i = tid; i < sc.a_n_unbounded; i += THREADS) l_unb[i] = sc.a_unbounded[i];
        uint16_t *l_leaf = (uint16_t *)(l_unb + sc.a_n_unbounded);
        const int nl = kd32 ? sc.kd_nleaf : sc.a_n_bleaf;
        for (int i = tid; i < nl; i += THREADS) l_leaf[i] = kd32 ? sc.a_leaf[i] : sc.a_bleaf[i];
        size_t off = (size_t)((char *)(l_leaf + nl) - (char *)lds);
        off = (off + 15) & ~(size_t)15;
        const int depth = kd32 ? (sc.a_kd_depth > 0 ? sc.a_kd_depth : 1) : 1;
        W = coop_carve((char *)lds + off + (size_t)(tid >> 6) * COOP_WAVE_BYTES(depth));
        A.sbox = l_sbox; A.nodes = l_nodes; A.leaf_surfs = l_leaf; A.always = l_alw; A.unbounded = l_unb;
        A.n_always = na; A.n_unbounded = sc.a_n_unbounded; A.n_surf = S; A.has_kd = 1;
#pragma unroll
        for (int i = 0; i < 6; ++i) A.root[i] = kd32 ? sc.a_root[i] : sc.a_broot[i];
        A.delta = sc.a_delta;
#pragma unroll
        for (int i = 0; i < 3; ++i) { A.cen[i] = sc.a_cen[i]; A.slo[i] = sc.a_slo[i]; A.shi[i] = sc.a_shi[i]; }
    }
    __syncthreads();

    // this wave's slice of the ray-id range
    const long long n_waves = (long long)gridDim.x * (THREADS >> 6);
    const long long wave = (long long)blockIdx.x * (THREADS >> 6) + (tid >> 6);
    const long long chunk = (P.n + n_waves - 1) / n_waves;
    long long next = wave * chunk;
    long long end = next + chunk;
    if (end > P.n) end = P.n;
    if (next > end) next = end;

    bool alive = false;       // the lane holds a ray that still needs its segment
    bool prepared = false;    // ... and the ray has candidates: it takes part in the search below
    double px = 0, py = 0, pz = 0, dx = 0, dy = 0, dz = 0, e = 0, ref = 1.0, wl = 0.0;
    unsigned long long rid = 0;
    int bounce = 0;
    int prev = S;              // surface the ray left (transfer matrix); S = the source
    double nseg = 0.0, nhit = 0.0;
    double tb = TRC_INF;      // best hit among the surfaces tested inline (unbounded ones)
    int sb = -1;
    bool in = false, walking = false;
    float tmin = 0.0f, tmax = 0.0f;
    unsigned alw_mask = 0;    // always-relevant surfaces whose box the ray crosses (first 32 of them; the rest always pass)
    trc_ray32 r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int stride = sc.stride;
    const double *extra = sc.extra;

    for (;;) {
        // ================= refill + prepare: up to 3 passes =================
        for (int pass = 0; pass < 3; ++pass) {
            unsigned long long need = __ballot(!alive);
            if (next < end && need) {
                long long id = next + __popcll(need & lt_mask);
                if (!alive && id < end) {
                    fast_new_ray<-1, SPEC, MEGA_SUN, MEGA_LAMP>(P, buie, id, px, py, pz, dx, dy, dz, e, ref, wl, rid);
                    bounce = 0;
                    prev = S;
                    alive = true;
                    prepared = false;
                }
                next += __popcll(need);
            }
            if (!__ballot(alive && !prepared)) break;
            if (alive && !prepared) {
                tb = TRC_INF;
                sb = -1;
                const double vx = px, vy = py, vz = pz;   // names used by TRC_TEST_EXACT
                for (int k = 0; k < A.n_unbounded; ++k) TRC_TEST_EXACT(A.unbounded[k]);
                double t0;
                in = trc_ray32_prepare(A.slo, A.shi, A.cen, px, py, pz, dx, dy, dz, &r, &t0);
                walking = false;
                alw_mask = 0;
                bool cand = false;
                if (in) {
                    walking = trc_kd32_root(A.root, r, &tmin, &tmax);
                    for (int k = 0; k < A.n_always; ++k) {
                        const float *b = A.sbox + 6 * (size_t)A.always[k];
                        bool bounded = !(b[3] == TRC_INF && b[0] == -TRC_INF);
                        if (bounded && (k >= 32 || trc_box_hit32(b, r))) { if (k < 32) alw_mask |= 1u << k; cand = true; }
                    }
                    cand = cand || walking;
                }
                if (cand || sb >= 0) {
                    prepared = true;
                } else {
                    nseg += 1.0;        // the segment hits nothing: finished, the lane can be refilled in the next pass
                    alive = false;
                }
            }
        }
        if (!__ballot(alive)) {
            if (next >= end) break;
            continue;
        }

        // ================= search (wave-cooperative; every lane takes part) =================
        W.best_t[lane] = (unsigned long long)__double_as_longlong(TRC_INF);
        W.best_s[lane] = 0x7FFFFFFF;
        W.dirty[lane] = 0;
        CoopRay ray;
        ray.px = px; ray.py = py; ray.pz = pz; ray.dx = dx; ray.dy = dy; ray.dz = dz;
        int ecount = 0;   // wave-uniform
        const uint32_t me = (uint32_t)lane << 16;
        const bool searching = alive && prepared && in;
        {
            for (int k = 0; k < A.n_always; ++k) {
                bool hit = searching && (k >= 32 ? true : ((alw_mask >> k) & 1u) != 0);
                if (k >= 32) {
                    const float *b = A.sbox + 6 * (size_t)A.always[k];
                    hit = hit && !(b[3] == TRC_INF && b[0] == -TRC_INF) && trc_box_hit32(b, r);
                }
                coop_push_exact(W, ecount, hit, me | (uint32_t)A.always[k], ray, recs, stride, extra, lane);
            }
            bool walk = searching && walking;
            uint32_t node = 0;
            int sp = 0;
            unsigned cnt = 0;     // leaves listed since the last drain
            while (__ballot(walk)) {
                // up to four steps of this lane's walk per wave-level iteration (amortises the loop's wave-level checks)
#pragma unroll 1
                for (int rep = 0; rep < 4 && walk && cnt < COOP_LEAFCAP; ++rep) {
                    uint32_t w0 = A.nodes[2 * node], w1 = A.nodes[2 * node + 1];
                    if ((w1 & 3u) != 3u) {
                        bool push;
                        uint32_t na;
                        float pt;
                        node = trc_kd32_step(w0, w1, r, A.delta, tmin, &tmax, &push, &na, &pt);
                        if (push) {
                            // stack entry: (node << 18) | (axis code << 16) | interval end as the upper half of a float32
                            // rounded UP (the interval only ever grows: conservative)
                            uint32_t bts = __float_as_uint(pt);
                            uint32_t hb = (bts >> 16) + ((bts & 0xFFFFu) ? 1u : 0u);
                            W.stack[sp * 64 + lane] = (na << 16) | (hb & 0xFFFFu);
                            ++sp;
                        }
                    } else {
                        if ((w1 >> 2) != 0u) { W.lst[cnt * 64 + lane] = (uint16_t)node; ++cnt; }
                        if (sp == 0) walk = false;
                        else {
                            --sp;
                            uint32_t en = W.stack[sp * 64 + lane];
                            uint32_t na = en >> 16;
                            node = na >> 2;
                            tmin = trc_kd32_pop_tmin(na & 3u, r, A.delta, tmax);
                            tmax = __uint_as_float(en << 16);
                        }
                    }
                }
                if (__ballot(cnt >= COOP_LEAFCAP)) {    // some lane's list is full: everybody drains
                    coop_drain_leaves(A, W, cnt, ecount, r, ray, recs, stride, extra, lane);
                    cnt = 0;
                }
            }
            coop_drain_leaves(A, W, cnt, ecount, r, ray, recs, stride, extra, lane);
        }
        coop_drain_exact(W, ecount, ray, recs, stride, extra, lane);

        // ================= per lane: result of the segment, shading =================
        if (alive) {
            double t = tb;
            int s = sb;
            double tq = __longlong_as_double((long long)W.best_t[lane]);
            int sq = W.best_s[lane];
            if (tq < TRC_INF && (tq < t || (tq == t && sq < s))) { t = tq; s = sq; }
            nseg += 1.0;
            prepared = false;
            if (s < 0) alive = false;
            else {
                nhit += 1.0;
                alive = fast_shade<true, false, CHART>(P, recs, l_tally, t, s, px, py, pz, dx, dy, dz, e, ref, wl, rid, bounce, prev);
            }
        }
        WAVE_SYNC();
    }

    // ---- flush ----
    nseg = wave_sum(nseg);
    nhit = wave_sum(nhit);
    if (lane == 0) { atomicAdd(&l_tally[3 * S], nseg); atomicAdd(&l_tally[3 * S + 1], nhit); }
    __syncthreads();
    flush_sums<THREADS>(sc.tally, l_tally, 3 * S + 2, nullptr, 0, S);
}
