// trc_shade.hip -- the shading stage of the streaming engine, split by optics class.
//
// k_s_shade (trc_stream.inc) carries every optics kind of optics_callables.py in one kernel: 243-256 registers, two waves per SIMD,
// more than half of its wave cycles waiting.  The registers are not held by any one kind -- a mirror with slope error
// (optics_callables.py:214-269 on ray_trace_utils/vector_manipulations.py:56-74) needs 66 -- but by the union of them and by what
// was built around them to live with two waves (entries and ray records of the next two hits fetched ahead in registers).
// Here one kernel per CLASS of optics walks the bounce's hit list and takes the hits on surfaces of its class; what a class does
// not need is not compiled into its kernel (trc_shade_k<KINDS, false>), nothing is fetched ahead, and the tables the host passes
// are few: the instances fit 128 registers and less, so a CU holds sixteen waves of them and their loads hide each other.
//
//   TRC_CLS_MIRROR    Transparent, Reflective, OneSidedReflective, RealReflective, OneSidedRealReflective (:93-140, :195-269, :492-504)
//   TRC_CLS_DIFFUSE   Lambertian, LambertianSpecular, SemiLambertian, Reflective_spectral and the table-driven
//                     Lambertian_directional_axisymmetric_piecewise family (:143-193, :331-391, :427-487, :506-585), and
//                     FresnelConductorHomogenous (:1536-1558: a mirror whose reflectance comes from a tabulated complex index -- the metal
//                     ring of the cavity receiver, 4.5 % of its hits, was the only reason for a third kernel and a third list there)
//   (TRC_CLS_GENERAL  everything else stays with k_s_shade)
//
// Per hit the arithmetic is the one of the other engines: trc_normal, trc_shade_k = trc_shade with the other kinds left out.
#include "trc_device.h"

// FLATN: every surface of the scene is flat (its normal is the z axis of its frame, flat_surface.py:84-91)
// LDS:   tallies, records, optics parameters, flux-map tables, flags (and the optics tables for the DIFFUSE class) are staged in
//        LDS -- all of them or none, so that every access has a known address space (see k_s_shade)
// CHART: the flux maps may bin in the charts other than XY (record_hit, trc_device.h)
template <int CLS, bool FLATN, bool LDS, bool SPEC = false, bool CHART = false>
__global__ __launch_bounds__(SHC_THREADS) void k_s_shade_c(StreamParams S) {
    extern __shared__ double lds[];
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    constexpr unsigned KINDS = CLS == TRC_CLS_MIRROR ? TRC_CLS_MIRROR_KINDS : TRC_CLS_DIFFUSE_KINDS;
    // (the image of TRC_IMG_LEAN / TRC_IMG_LEAN_MIRROR, trc_shade_lds_layout in trc_bounds.h, by which the host sizes the launch: carved here
    // in its order -- through a shared staging routine most instances spilled more scalar registers, profiles/shade_layout.txt)
    DScene L = sc;
    // (one of TALLY_PARTS copies of the tally buffer per workgroup, also where the tables are beyond LDS and the sums are added per
    // hit: a single copy -- 2.4 MB for a mesh of 1e5 faces, against 38 MB -- measured slower, 33.8 against 26.9 ms per 1e7 rays)
    L.tally = W.tally_part + (size_t)(blockIdx.x % TALLY_PARTS) * (size_t)W.tally_n;
    double *l_tally = lds;
    double *cur = lds + (LDS ? 3 * Sn + 2 : 2);
    for (int i = threadIdx.x; i < (LDS ? 3 * Sn + 2 : 2); i += blockDim.x) l_tally[i] = 0.0;
    if (LDS) {
        double *l_recs = cur; cur += Sn * sc.stride;
        for (int i = threadIdx.x; i < Sn * sc.stride; i += blockDim.x) l_recs[i] = sc.recs[i];
        double *l_opt = cur; cur += 8 * Sn;
        for (int i = threadIdx.x; i < 8 * Sn; i += blockDim.x) l_opt[i] = sc.opt[i];
        double *l_edges = cur; cur += sc.n_fm_edges;
        for (int i = threadIdx.x; i < sc.n_fm_edges; i += blockDim.x) l_edges[i] = sc.fm_edges[i];
        FluxMapDev *l_fms = (FluxMapDev *)cur; cur += (sc.n_fm * sizeof(FluxMapDev) + 7) / 8;
        for (int i = threadIdx.x; i < sc.n_fm; i += blockDim.x) l_fms[i] = sc.fms[i];
        int32_t *l_fm_of = (int32_t *)cur;
        int32_t *l_flags = l_fm_of + Sn;
        for (int i = threadIdx.x; i < Sn; i += blockDim.x) { l_fm_of[i] = sc.fm_of_surf ? sc.fm_of_surf[i] : -1; l_flags[i] = sc.sflags[i]; }
        L.recs = l_recs; L.opt = l_opt; L.fm_edges = l_edges; L.fms = l_fms; L.fm_of_surf = l_fm_of; L.sflags = l_flags;
        cur = (double *)(((uintptr_t)(l_flags + Sn) + 7) & ~(uintptr_t)7);
        if (CLS != TRC_CLS_MIRROR) {        // (no mirror reads a table)
            double *l_extra = cur; cur += sc.n_extra;
            for (int i = threadIdx.x; i < sc.n_extra; i += blockDim.x) l_extra[i] = sc.extra[i];
            L.extra = l_extra;
        }
    }
    double *l_fm = nullptr;         // private copy of the flux-map bins (S.lds_fm_bins of them)
    if (S.lds_fm_bins > 0) {
        l_fm = cur; cur += S.lds_fm_bins;
        for (int i = threadIdx.x; i < S.lds_fm_bins; i += blockDim.x) l_fm[i] = 0.0;
    }
    const double src_energy = P.src ? P.src->energy : 0.0;
    __syncthreads();
    long long nh = (long long)W.cnt[S.hl_cn];
    if (nh > S.hl_room) nh = S.hl_room;     // never read beyond the allocation, whatever the counter says
    const long long padded = (nh + 63) & ~63ll;
    const unsigned wave_g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk ca = S.static_first ? chunk_init_static_at(S.chunk_act, (unsigned long long)S.act_base0 + (unsigned long long)wave_g * S.chunk_act) : chunk_init(S.chunk_act);
    // this wave's open chunk of the scene's hit buffer, carried over from earlier launches (see k_s_shade)
    WaveChunk hc = chunk_init(S.chunk_hitbuf);
    if (P.capture && wave_g < SHADE_MAX_WAVES) hit_chunk_resume(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    unsigned n_hit = 0, n_alive = 0;
    // AHEAD: the instance can finish the next segment of a continued ray itself (S.ahead, set by trc_stream_form_ahead: the next
    // bounce is k_s_bounce<1, .., FRESH = false> with split_terminal == 2 and the scene's clear cones).  A mirror's ray inside the
    // clear cone of the tile it leaves meets no surface the grid lists, so k_s_bounce would only test the surfaces set apart and
    // finish a hit on one that ends every ray in place: neither needs a ray record in memory, and the ray is in registers here.
    constexpr bool AHEAD = CLS == TRC_CLS_MIRROR && FLATN && LDS && !SPEC && !CHART;
    unsigned n_ahead = 0, n_ahead_hit = 0;
    const int bounce0 = S.bounce_no;          // every ray of a launch is at the same bounce
    const bool aux_in = !P.src || bounce0 > 0;     // fresh rays of a source carry (energy, 1, 0): nothing was written for them
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        uint32_t slot = SQ_INVALID, hs = SQ_INVALID;
        double t = TRC_INF;
        SRayGeo g;
        g.px = g.py = g.pz = g.dx = g.dy = 0.0; g.dz = 1.0; g.head = SQ_INVALID; g.idx = 0u; g.tail = 0ull;
        bool have = false;
        int as = -1;                         // (AHEAD) the surface this lane's ray hit on the segment finished here, with its energy
        double ae = 0.0;
        if (i < nh) { slot = S.hl_slot[i]; hs = S.hl_surf[i]; t = S.hl_t[i]; }
        bool mine = false;
        int s = 0, fl = 0;
        if (slot != SQ_INVALID) {
            if (hs == SQ_INVALID) {         // general path
                g = W.geo[slot];
                have = true;
                t = TRC_INF;
                s = 0x7FFFFFFF;
                nearest_linked(W.q3n, g.head, t, s);
            } else s = (int)hs;
            if ((unsigned)s < (unsigned)Sn) {
                fl = L.sflags[s];
                const int cls = (fl >> TRC_SURF_CLS_SHIFT) & TRC_SURF_CLS_MASK;
                mine = (S.shade_term_cls >= 0 && (fl & TRC_SURF_TERMINAL)) ? (S.shade_term_cls == CLS) : (cls == CLS);
            }
            if (mine && !have) g = W.geo[slot];
        }
        const unsigned long long my_lanes = __ballot(mine);
        if (!my_lanes) continue;            // the unused tail of a chunk of the list, or hits of other classes only
        bool alive = false;
        int ts = -1;                         // the surface this lane's hit is tallied on, with absorbed and incident energy
        double tea = 0.0, tei = 0.0;
        if (mine) {
            n_hit += 1;
            const int prev = bounce0 == 0 ? Sn : (int)((uint32_t)(g.tail >> 32) & ~SQ_SKIP_SELF);      // the surface the ray left; Sn = the source
            double e = src_energy, wl = 0.0, ref0 = 1.0;
            // a source with a spectrum: the wavelength of a fresh ray is drawn at its first hit (the mirror class does not read it, but
            // hands it on to the ray's next record)
            if (SPEC && !aux_in)
                trc_spectrum_of(P.spec, P.seed, P.ray_offset + (unsigned long long)(S.base + (long long)g.idx), &wl, &ref0);
            if (aux_in) { e = W.aux[slot].e; if (CLS != TRC_CLS_MIRROR) wl = W.aux[slot].wl; }
            const double *rec = L.recs + (size_t)s * sc.stride;
            const double hx = g.px + t * g.dx, hy = g.py + t * g.dy, hz = g.pz + t * g.dz;
            double ox = g.dx, oy = g.dy, oz = g.dz, e_out = 0.0;
            if (!(S.shade_term_cls >= 0 && (fl & TRC_SURF_TERMINAL))) {
                double nx, ny, nz;
                if (FLATN) {
                    if (!trc_gm_is_flat(trc_rec_gm_kind(rec))) __builtin_unreachable();
                }
                trc_normal(rec, hx, hy, hz, g.dx, g.dy, g.dz, &nx, &ny, &nz);
                trc_ray_out out[2];
                const unsigned long long rid = P.rid ? P.rid[S.base + (long long)g.idx] : (P.ray_offset + (unsigned long long)(S.base + (long long)g.idx));
                trc_shade_k<KINDS, false>(trc_rec_opt_kind(rec), L.opt + (size_t)s * 8, L.extra, trc_rec_extra_off(rec), trc_rec_extra_len(rec),
                                          rec[2], rec[5], rec[8], g.dx, g.dy, g.dz, e, 1.0, wl, 0.0, nx, ny, nz, P.seed, rid, (uint32_t)(bounce0 + 1), out);
                ox = out[0].dx; oy = out[0].dy; oz = out[0].dz; e_out = out[0].e;
            }
            const double e_abs = e - e_out;
            record_hit<LDS, CHART>(L, l_tally, s, e, e_abs, hx, hy, hz, g.dx, g.dy, g.dz, P.capture != 0, prev, &hc, l_fm, false, true);
            ts = s; tea = e_abs; tei = e;        // (the three sums of the surface: below, per wave)
            if (e_out > P.min_energy) {                               // tracer_engine.py:242
                if (bounce0 + 1 >= P.reps) {                          // still alive after the last iteration
                    atomicAdd(&sc.counters[3], 1ull);
                    atomicAdd(sc.energy_left, e_out);
                    if (P.flags & TRC_TRACE_KEEP_LAST) {
                        const unsigned long long q = atomicAdd(&sc.counters[2], 1ull);
                        if ((long long)q < P.last_cap) {
                            P.lx[q] = hx; P.ly[q] = hy; P.lz[q] = hz;
                            P.ldx[q] = ox; P.ldy[q] = oy; P.ldz[q] = oz; P.le[q] = e_out;
                        }
                    }
                } else {
                    bool ahead = false;             // (AHEAD) the ray's next segment is finished here: it does not go to k_s_bounce
                    if constexpr (AHEAD) {
                        // What k_s_bounce<1, .., FRESH = false> (trc_stream.inc) does for a ray that does not walk, in its words and
                        // on the same values: the float32 ray, the root box, the clear cone of the tile left, then the surfaces set
                        // apart in ascending order -- box, oriented box, exact test, nearest with the lowest index on equal t.
                        // Whoever changes one of the two changes the other.
                        if (S.ahead && S.clear_tab && leaves_flat(rec, hx, hy, hz, ox, oy, oz)) {
                            trc_ray32 r;
                            double t0 = 0.0;
                            bool clear = trc_ray32_prepare(sc.a_slo, sc.a_shi, sc.a_cen, hx, hy, hz, ox, oy, oz, &r, &t0) && t0 == 0.0;
                            float tmin = 1.0f, tmax = 0.0f;
                            if (clear && trc_kd32_root(sc.a_groot, r, &tmin, &tmax)) {
                                // (the oriented box of the surface hit: a read from global memory per lane, the table stays in L2)
                                const int tile = trc_clear_tile(sc.a_obb + (size_t)TRC_OBB_STRIDE * s, TRC_CLEAR_T, r.ox, r.oy, r.oz);
                                const float4 cone = ((const float4 *)S.clear_tab)[(size_t)s * (TRC_CLEAR_T * TRC_CLEAR_T) + tile];
                                clear = trc_clear_inside(cone.x, cone.y, cone.z, cone.w, r.dx, r.dy, r.dz);
                            }
                            if (clear) {
                                double tb = TRC_INF;
                                int sb = 0x7FFFFFFF;
                                for (int k = 0; k < sc.a_g_napart; ++k) {        // (uniform indices: boxes and records of the same surfaces for every lane)
                                    const int sidx = sc.a_gapart[k];
                                    const float *b = sc.a_sbox + 6 * (size_t)sidx;
                                    if ((b[3] == TRC_INF && b[0] == -TRC_INF) || sidx == s) continue;
                                    if (!(trc_box_hit32(b, r) && trc_obb_hit32(sc.a_obb + (size_t)TRC_OBB_STRIDE * sidx, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz))) continue;
                                    const double *rec2 = L.recs + (size_t)sidx * sc.stride;
                                    const double t2 = trc_intersect_flat(trc_rec_gm_kind(rec2), rec2, sc.extra, hx, hy, hz, ox, oy, oz);
                                    if (t2 > 0.0 && t2 < TRC_INF && (t2 < tb || (t2 == tb && sidx < sb))) { tb = t2; sb = sidx; }
                                }
                                if (sb == 0x7FFFFFFF) ahead = true;                     // nothing is hit: the ray leaves the scene
                                else if (L.sflags[sb] & TRC_SURF_TERMINAL) {            // ... or ends on a surface that ends every ray
                                    ahead = true;
                                    as = sb; ae = e_out;
                                    n_ahead_hit += 1;
                                    record_hit<LDS, CHART>(L, l_tally, sb, e_out, e_out, hx + tb * ox, hy + tb * oy, hz + tb * oz, ox, oy, oz, P.capture != 0, s, &hc, l_fm, false, true);
                                }
                            }
                            if (ahead) n_ahead += 1;
                        }
                    }
                    if (!ahead) {
                    alive = true;
                    SRayGeo go;
                    go.px = hx; go.py = hy; go.pz = hz; go.dx = ox; go.dy = oy; go.dz = oz;
                    go.head = SQ_INVALID;          // ready for the next bounce's search
                    go.idx = g.idx;
                    uint32_t pw = (uint32_t)s;
                    if (leaves_flat(rec, hx, hy, hz, ox, oy, oz)) pw |= SQ_SKIP_SELF;
                    go.tail = sray_tail(bounce0 + 1, pw);
                    W.geo[slot] = go;
                    if (aux_in) W.aux[slot].e = e_out;        // (index and wavelength stay as they are: no optics of these classes changes them)
                    else { SRayAux ao; ao.e = e_out; ao.ref = SPEC ? ref0 : 1.0; ao.wl = SPEC ? wl : 0.0; ao.pad = 0.0; W.aux[slot] = ao; }
                    }
                }
            }
        }
        {
            // The three sums per surface: lanes that share the surface of the first lane still to be served are summed in registers
            // and added once while at least 8 of them do (see k_s_shade); the others add for themselves.  In LDS, or -- a scene whose
            // tables do not fit it: a mesh -- in the workgroup's copy of the tally buffer in global memory, where 64 lanes on one
            // word are served one after the other (the lid over the mesh of 1e5 faces: 10 ms per 5e6 hits on it).
            // (tally_by_wave, trc_device.h, in this kernel's own text: with the helper the dish configuration of the bench measured
            // slower, profiles/shade_layout.txt)
            double *tl = LDS ? l_tally : L.tally;
            unsigned long long todo = (!LDS || Sn <= 64) ? __ballot(ts >= 0) : 0ull;
            for (int round = 0; round < 6 && todo; ++round) {
                const int s0 = __shfl(ts, __ffsll((long long)todo) - 1, 64);
                const bool in = ts == s0;
                const unsigned long long m = __ballot(in);
                if (__popcll(m) < 8) break;
                const double a = wave_sum(in ? tea : 0.0), b = wave_sum(in ? tei : 0.0);
                if (lane_id() == 0) { atomicAdd(&tl[s0], a); atomicAdd(&tl[Sn + s0], b); atomicAdd(&tl[2 * Sn + s0], (double)__popcll(m)); }
                if (in) ts = -1;
                todo &= ~m;
            }
            if (ts >= 0) { atomicAdd(&tl[ts], tea); atomicAdd(&tl[Sn + ts], tei); atomicAdd(&tl[2 * Sn + ts], 1.0); }
        }
        // hc was advanced by the lanes with a hit only -- and once more by those whose ray hit on the segment finished here (AHEAD):
        // theirs is the newest state
        unsigned long long hc_lanes = my_lanes;
        if constexpr (AHEAD) { const unsigned long long al = __ballot(as >= 0); if (al) hc_lanes = al; }
        if (P.capture) chunk_rebroadcast(hc, __ffsll((long long)hc_lanes) - 1);
        if constexpr (AHEAD) {
            // the hits of the segments finished here: a tally round of their own, the form k_s_bounce has for the hits it finishes
            // (the lanes on the first lane's surface -- the receiver -- are summed in registers and added once)
            const unsigned long long tl = __ballot(as >= 0);
            if (tl) {
                const int s0 = __shfl(as, __ffsll((long long)tl) - 1, 64);
                const bool in = as == s0;
                const double cnt = (double)__popcll(__ballot(in));
                const double es = wave_sum(in ? ae : 0.0);
                if (lane_id() == 0) { atomicAdd(&l_tally[s0], es); atomicAdd(&l_tally[Sn + s0], es); atomicAdd(&l_tally[2 * Sn + s0], cnt); }
                if (as >= 0 && !in) { atomicAdd(&l_tally[as], ae); atomicAdd(&l_tally[Sn + as], ae); atomicAdd(&l_tally[2 * Sn + as], 1.0); }
            }
        }
        const unsigned long long q = chunk_append(&W.cnt[CN(CW_ACT_OUT)], ca, alive, S.act_out, W.act_room);
        if (alive) { if ((long long)q < W.act_room) S.act_out[q] = slot; else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; n_alive += 1; }
    }
    chunk_close(ca, S.act_out, W.act_room);
    if (P.capture && wave_g < SHADE_MAX_WAVES && lane_id() == 0) hit_chunk_suspend(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    flush_counts<true>(l_tally + (LDS ? 3 * Sn : 0), n_hit, n_alive, &W.cnt[CN(CW_HITS)], &W.cnt[CN(CW_CLS_HITS + CLS)], &W.cnt[CN(CW_ALIVE)]);
    if constexpr (AHEAD) {
        // the rays finished ahead and their hits, through the same two spare words once thread 0 has taken the counts above out of them:
        // the hits are k_s_bounce's (CW_HITS, CW_TERM_HITS, no class word), the rays are missing from CW_ALIVE
        if (S.ahead) {          // (the same for every thread of the launch)
            double *spare = l_tally + 3 * Sn;
            __syncthreads();
            if (threadIdx.x == 0) spare[0] = spare[1] = 0.0;
            __syncthreads();
            const double a = wave_sum((double)n_ahead), h = wave_sum((double)n_ahead_hit);
            if (lane_id() == 0 && a > 0.0) { atomicAdd(&spare[0], a); atomicAdd(&spare[1], h); }
            __syncthreads();
            if (threadIdx.x == 0 && spare[0] > 0.0) {
                const unsigned long long hh = (unsigned long long)(spare[1] + 0.5);
                atomicAdd(&W.cnt[CN(CW_AHEAD)], (unsigned long long)(spare[0] + 0.5));
                if (hh) { atomicAdd(&W.cnt[CN(CW_AHEAD_HITS)], hh); atomicAdd(&W.cnt[CN(CW_HITS)], hh); atomicAdd(&W.cnt[CN(CW_TERM_HITS)], hh); }
            }
        }
    }
    flush_sums(L.tally, l_tally, LDS ? 3 * Sn : 0, l_fm, S.lds_fm_bins, Sn);
}

// ---------------------------------------------------------------------------------------------------------------
// k_s_shade_x: the shading stage for rays that carry more than the record of the fast engine -- the imaginary part of a complex
// refractive index, the scene's materials evaluated at the ray's wavelength (Refractive / RefractiveAbsorbant,
// optics_callables.py:726-858, :908-944), a sampled spectrum (LambertianReceiver's polychromatic form, :393-425).  One kernel for
// every optics kind (trc_shade_x = trc_shade + the kinds that read those), all hits of the bounce's list; nothing fetched ahead.
//   Im of the index       the fourth word of the ray's SRayAux, from the bundle's column for a ray not shaded yet
//   materials, sample     do not change along a ray: read from the bundle's columns by the ray's number (SRayGeo.idx)
//   wavelengths
//   spectrum              one value per sample and slot in CarryIn.slot_spec (sample-major, `room` apart); from the bundle's column at the
//                         first interaction.  Scaled per sample by 1 - absorptance(theta, lambda_w) at a polychromatic wall, as a
//                         whole by the optics' factor elsewhere -- what k_ord_bounce does for the ordered engine.
// Given bundles only (a source descriptor makes rays of energy, index 1 and no wavelength).
// SPLIT: the scene has optics that send two rays on from a hit (RefractiveHomogenous(single_ray=False) and its family,
//        optics_callables.py:600-724, :726-858): the reflected and the refracted ray of the reference's deterministic Fresnel mode.
//        The hit is recorded once, with what neither ray takes along as the absorbed energy (k_ord_bounce); each ray is culled,
//        counted or kept on its own.  The first goes back into the hit's slot, the second takes a new slot of the ray table
//        (CN(CW_SLOTS): slots are never recycled in such a call, the host grows the table between bounces), and both are appended to
//        the next active list.  The second ray's Philox stream is trc_child_rid(parent's, event) as in the ordered engine, so the
//        stream of the ray in a slot is kept in CarryIn.slot_rid: read from the second bounce on, written for every ray that goes on.
//        What a ray carries (Im of its index, its spectrum) goes with both.  Given bundles and source descriptors (without spectrum).
// MAT:   the scene's tabulated materials are on the device (CarryIn.mat_tab, trc_scene_set_materials) and the call brings no rows of
//        them: a hit between materials evaluates both at the ray's wavelength (trc_shade_xt), and the ray of a source descriptor
//        draws its wavelength from the source's spectrum at its first hit, with the spectrum's index and no imaginary part -- as
//        the lean SPEC kernels do (k_s_shade_c).  The children of a SPLIT hit inherit the wavelength like every other ray.
//
// k_s_shade_p: the same stage for a source that CARRIES its spectrum (TRC_SPECTRUM_CARRIED): every ray is born with the W points of
// the source's table as its sample wavelengths and src->energy * val[w] as its spectrum, so neither is a per-ray column:
//   sample wavelengths    the grid wl[W] of the call's packed spectrum (FastParams.spec), stride 1, at every bounce
//   spectrum              at a ray's first hit the birth vector src->energy * val[w], from the second on the slot table as above
//   index                 spec[2]; no wavelength and no Im of the index is drawn or read
// Its LDS instances stage grid and birth vector behind the image of TRC_IMG_SHADE_X (the host counts them into the image: all tables
// or none, trc_stream_form_shade), and -- when they fit too (CarryIn.poly_cells) -- the lambda cell and weight of every sample in
// every polychromatic wall's table, which no ray changes; the other instances read grid and values from the packed spectrum and
// search per hit.  At a polychromatic wall the theta cell is found once per hit and every sample is blended by trc_interp2_at, the
// expression of trc_interp2: one evaluation per sample serves the integral and the spectrum that goes on (a captured hit, whose
// place in the hit buffer is known only after its energy, evaluates once more for its 3 W columns and writes both then).
// With TRC_TRACE_KEEP_LAST the rays left write their spectra too (CarryIn.last_spec).  Both families are one body: POLY.
template <bool LDS, bool CHART, bool SPLIT, bool MAT, bool POLY>
__device__ __forceinline__ void shade_x_body(const StreamParams &S) {
    extern __shared__ double lds[];
    const FastParams &P = S.P;
    const DScene &sc = P.sc;
    const StreamWs &W = S.W;
    const int Sn = sc.n_surf;
    if (W.cnt[CN(CW_OVERFLOW)]) return;
    DScene L = sc;          // (the image of TRC_IMG_SHADE_X, carved here in its order: see k_s_shade_c)
    L.tally = W.tally_part + (size_t)(blockIdx.x % TALLY_PARTS) * (size_t)W.tally_n;
    double *l_tally = lds;
    double *cur = lds + (LDS ? 3 * Sn + 2 : 2);
    for (int i = threadIdx.x; i < (LDS ? 3 * Sn + 2 : 2); i += blockDim.x) l_tally[i] = 0.0;
    if (LDS) {
        double *l_recs = cur; cur += Sn * sc.stride;
        for (int i = threadIdx.x; i < Sn * sc.stride; i += blockDim.x) l_recs[i] = sc.recs[i];
        double *l_opt = cur; cur += 8 * Sn;
        for (int i = threadIdx.x; i < 8 * Sn; i += blockDim.x) l_opt[i] = sc.opt[i];
        double *l_edges = cur; cur += sc.n_fm_edges;
        for (int i = threadIdx.x; i < sc.n_fm_edges; i += blockDim.x) l_edges[i] = sc.fm_edges[i];
        FluxMapDev *l_fms = (FluxMapDev *)cur; cur += (sc.n_fm * sizeof(FluxMapDev) + 7) / 8;
        for (int i = threadIdx.x; i < sc.n_fm; i += blockDim.x) l_fms[i] = sc.fms[i];
        int32_t *l_fm_of = (int32_t *)cur;
        int32_t *l_flags = l_fm_of + Sn;
        for (int i = threadIdx.x; i < Sn; i += blockDim.x) { l_fm_of[i] = sc.fm_of_surf ? sc.fm_of_surf[i] : -1; l_flags[i] = sc.sflags[i]; }
        L.recs = l_recs; L.opt = l_opt; L.fm_edges = l_edges; L.fms = l_fms; L.fm_of_surf = l_fm_of; L.sflags = l_flags;
        cur = (double *)(((uintptr_t)(l_flags + Sn) + 7) & ~(uintptr_t)7);
        double *l_extra = cur; cur += sc.n_extra;
        for (int i = threadIdx.x; i < sc.n_extra; i += blockDim.x) l_extra[i] = sc.extra[i];
        L.extra = l_extra;
    }
    double *l_fm = nullptr;
    if (S.lds_fm_bins > 0) {
        l_fm = cur; cur += S.lds_fm_bins;
        for (int i = threadIdx.x; i < S.lds_fm_bins; i += blockDim.x) l_fm[i] = 0.0;
    }
    const double src_energy = P.src ? P.src->energy : 0.0;
    const CarryIn &C = S.carry;
    // (POLY) the sample grid and the values of the call's packed spectrum; in the LDS instances grid and birth vector as offsets into
    // lds[], so that every access has a known address space, and behind them the walls' lambda cells (weights, cells, surface -> wall)
    const int pW = POLY ? C.n_spec : 0;
    const double *g_wl = POLY ? P.spec + 3 : nullptr, *g_val = POLY ? P.spec + 3 + pW : nullptr;
    int o_wl = 0, o_birth = 0, o_cw = 0;
    const int32_t *l_ci = nullptr, *l_wall = nullptr;
    int n_cells = 0;
    if constexpr (POLY && LDS) {
        o_wl = (int)(cur - lds); o_birth = o_wl + pW; cur += 2 * pW;
        for (int i = threadIdx.x; i < pW; i += blockDim.x) { lds[o_wl + i] = g_wl[i]; lds[o_birth + i] = src_energy * g_val[i]; }
        n_cells = C.poly_cells;
        if (n_cells > 0) {
            o_cw = (int)(cur - lds); cur += (size_t)n_cells * pW;
            int32_t *ci = (int32_t *)cur; cur += ((size_t)n_cells * pW + 1) / 2;
            int32_t *wall = (int32_t *)cur; cur += (Sn + 1) / 2;
            __syncthreads();            // (the records and tables the cells are made from)
            if (threadIdx.x == 0) {
                int k = 0;
                for (int s = 0; s < Sn; ++s)
                    wall[s] = (trc_rec_opt_kind(L.recs + (size_t)s * sc.stride) == TRC_OPT_LAMBERTIAN_POLYCHROMATIC && k < n_cells) ? k++ : -1;
            }
            __syncthreads();
            for (int s = 0; s < Sn; ++s) {
                const int p = wall[s];
                if (p < 0) continue;
                const double *tab = L.extra + trc_rec_extra_off(L.recs + (size_t)s * sc.stride);
                const int nt = (int)tab[0], nl = (int)tab[1];
                for (int w = threadIdx.x; w < pW; w += blockDim.x) {
                    double wlam;
                    ci[p * pW + w] = trc_grid_cell(tab + 2 + nt, nl, lds[o_wl + w], &wlam);
                    lds[o_cw + p * pW + w] = wlam;
                }
            }
            l_ci = ci; l_wall = wall;
        }
    }
    __syncthreads();
    long long nh = (long long)W.cnt[S.hl_cn];
    if (nh > S.hl_room) nh = S.hl_room;
    const long long padded = (nh + 63) & ~63ll;
    const unsigned wave_g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    WaveChunk ca = S.static_first ? chunk_init_static_at(S.chunk_act, (unsigned long long)S.act_base0 + (unsigned long long)wave_g * S.chunk_act) : chunk_init(S.chunk_act);
    WaveChunk hc = chunk_init(S.chunk_hitbuf);
    if (P.capture && wave_g < SHADE_MAX_WAVES) hit_chunk_resume(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    WaveChunk cs = chunk_init(S.chunk_slot);        // (SPLIT) slots of the ray table for the second ray of a hit
    unsigned n_hit = 0, n_alive = 0;
    const int bounce0 = S.bounce_no;
    const bool aux_in = !P.src || bounce0 > 0;
    const int nW = C.slot_spec ? C.n_spec : 0;
    const double ref_src = POLY ? P.spec[2] : 1.0;      // (POLY) the index of the medium the source's rays start in
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        uint32_t slot = SQ_INVALID, hs = SQ_INVALID;
        double t = TRC_INF;
        if (i < nh) { slot = S.hl_slot[i]; hs = S.hl_surf[i]; t = S.hl_t[i]; }
        SRayGeo g;
        g.px = g.py = g.pz = g.dx = g.dy = 0.0; g.dz = 1.0; g.head = SQ_INVALID; g.idx = 0u; g.tail = 0ull;
        bool mine = false;
        int s = 0;
        if (slot != SQ_INVALID) {
            g = W.geo[slot];
            if (hs == SQ_INVALID) {         // general path
                t = TRC_INF;
                s = 0x7FFFFFFF;
                nearest_linked(W.q3n, g.head, t, s);
            } else s = (int)hs;
            mine = (unsigned)s < (unsigned)Sn;
        }
        const unsigned long long my_lanes = __ballot(mine);
        if (!my_lanes) continue;
        bool alive = false;
        bool alive1 = false;            // (SPLIT) the hit's second ray goes on, from slot1
        uint32_t slot1 = SQ_INVALID;
        int ts = -1;
        double tea = 0.0, tei = 0.0;
        if (mine) {
            n_hit += 1;
            const bool first = bounce0 == 0;
            const int prev = first ? Sn : (int)((uint32_t)(g.tail >> 32) & ~SQ_SKIP_SELF);
            const long long ray = S.base + (long long)g.idx;            // the ray's place in the bundle's columns
            double e = src_energy, ref = ref_src, wl = 0.0, ref_im = 0.0;
            if (aux_in) { const SRayAux a = W.aux[slot]; e = a.e; ref = a.ref; wl = a.wl; ref_im = a.pad; }
            if (!POLY && first) ref_im = C.ref_im ? C.ref_im[ray] : 0.0;
            const double *rec = L.recs + (size_t)s * sc.stride;
            double hx = g.px + t * g.dx, hy = g.py + t * g.dy, hz = g.pz + t * g.dz;
            double nx, ny, nz;
            trc_normal(rec, hx, hy, hz, g.dx, g.dy, g.dz, &nx, &ny, &nz);
            const double path = sqrt((hx - g.px) * (hx - g.px) + (hy - g.py) * (hy - g.py) + (hz - g.pz) * (hz - g.pz));
            trc_ray_ext X;
            X.ref_im = ref_im; X.W = nW; X.n_mat = (!MAT && C.mat) ? C.n_mat : 0; X.stride = P.n;
            X.mat = (!MAT && C.mat) ? C.mat + ray : nullptr;
            X.wl = (!POLY && nW) ? C.spec_wl + ray : nullptr;
            X.spec = (!POLY && nW) ? C.spec + ray : nullptr;
            long long spec_stride = P.n;                                 // ... of the spectrum as it reaches this hit
            if (nW && !first) { X.spec = C.slot_spec + slot; spec_stride = W.room; }
            // sample wavelength w and sample w of the spectrum that arrives: the bundle's columns with their strides, or (POLY) the
            // grid with stride 1 and, at the first hit, the birth vector
            auto wl_of = [&](int w) -> double {
                if constexpr (POLY) return LDS ? lds[o_wl + w] : g_wl[w];
                else return X.wl[(long long)w * P.n];
            };
            auto spec_of = [&](int w) -> double {
                if constexpr (POLY) { if (first) return LDS ? lds[o_birth + w] : src_energy * g_val[w]; }
                return X.spec[(long long)w * spec_stride];
            };
            // (POLY) a polychromatic wall: the theta cell of the hit, the wall's row of staged lambda cells (-1: searched), and
            // whether the spectrum that goes on is in the slot table already
            int p_it = 0, p_wall = -1;
            double p_wt = 0.0;
            bool p_done = false;
            auto poly_abs = [&](const double *tab, double th, int w, double xw) -> double {
                if constexpr (POLY) {
                    double wlam;
                    int il;
                    if (p_wall >= 0) { il = l_ci[p_wall * pW + w]; wlam = lds[o_cw + p_wall * pW + w]; }
                    else il = trc_grid_cell(tab + 2 + (int)tab[0], (int)tab[1], xw, &wlam);
                    return trc_interp2_at(tab, p_it, p_wt, il, wlam);
                } else return trc_poly_absorptance(tab, th, xw);
            };
            trc_ray_out out[2];
            double out_im[2], poly_th;
            unsigned long long rid = P.rid ? P.rid[ray] : (P.ray_offset + (unsigned long long)ray);
            if (SPLIT && !first) rid = C.slot_rid[slot];
            if (MAT && !aux_in) trc_spectrum_of(P.spec, P.seed, rid, &wl, &ref);     // (culled rays and misses never draw)
            // (sample wavelengths and spectrum have different strides once the spectrum lives in the slot table: the polychromatic
            // wall reads both, so its integral is taken here with the two strides, the optics get the wavelengths' stride)
            int n_out;
            if (nW && (POLY || !first) && trc_rec_opt_kind(rec) == TRC_OPT_LAMBERTIAN_POLYCHROMATIC) {
                // trc_shade_x's branch (optics_callables.py:406-425) with the spectrum read from the slot table (POLY: or the birth vector)
                out[0].blk = 0; out[1].blk = 1; out[0].back = out[1].back = 0.0; out[0].sf = out[1].sf = 1.0; out[0].shift = out[1].shift = 0.0;
                out[0].ref = ref;
                out_im[0] = out_im[1] = ref_im;
                const double dn = g.dx * nx + g.dy * ny + g.dz * nz;
                const double wx = dn * nx, wy = dn * ny, wz = dn * nz;
                const double th = acos(sqrt(wx * wx + wy * wy + wz * wz));
                const double *tab = L.extra + trc_rec_extra_off(rec);
                double en = 0.0, y0 = 0.0, x0 = 0.0;
                if constexpr (POLY) {
                    p_it = trc_grid_cell(tab + 2, (int)tab[0], th, &p_wt);
                    if (n_cells > 0) p_wall = l_wall[s];
                    // (a hit that is captured writes its spectrum with its 3 W columns, behind record_hit)
                    p_done = !(P.capture && C.hit_x && (L.sflags[s] & TRC_SURF_CAPTURE_HITS));
                }
                for (int w = 0; w < nW; ++w) {
                    const double xw = wl_of(w);
                    const double yw = spec_of(w) * (1.0 - poly_abs(tab, th, w, xw));
                    if (w > 0) en += (xw - x0) * (yw + y0) / 2.0;
                    x0 = xw; y0 = yw;
                    if (POLY && p_done) C.slot_spec[(long long)w * W.room + slot] = yw;
                }
                double u0, u1, ax, ay, az;
                trc_uniform_pair(P.seed, rid, (uint32_t)(bounce0 + 1), 0, &u0, &u1);
                trc_pillbox_dir_u(u0, u1, 1.57079632679489661923, &ax, &ay, &az);
                trc_rotation_to_z_apply(nx, ny, nz, ax, ay, az, &out[0].dx, &out[0].dy, &out[0].dz);
                out[0].e = en;
                poly_th = th;
                n_out = 1;
            } else if constexpr (MAT)
                n_out = trc_shade_xt(trc_rec_opt_kind(rec), L.opt + (size_t)s * 8, L.extra, trc_rec_extra_off(rec), trc_rec_extra_len(rec),
                                     rec[2], rec[5], rec[8], g.dx, g.dy, g.dz, e, ref, wl, path, nx, ny, nz, P.seed, rid, (uint32_t)(bounce0 + 1),
                                     X, C.mat_tab, out, out_im, &poly_th);
            else
                n_out = trc_shade_x(trc_rec_opt_kind(rec), L.opt + (size_t)s * 8, L.extra, trc_rec_extra_off(rec), trc_rec_extra_len(rec),
                                    rec[2], rec[5], rec[8], g.dx, g.dy, g.dz, e, ref, wl, path, nx, ny, nz, P.seed, rid, (uint32_t)(bounce0 + 1),
                                    X, out, out_im, &poly_th);
            const bool two = SPLIT && n_out == 2;       // (the other instances serve scenes none of whose optics sends two rays on)
            const bool volume = out[0].back > 0.0;          // scattered in the medium before the surface (see fast_shade)
            if (volume) { hx -= out[0].back * g.dx; hy -= out[0].back * g.dy; hz -= out[0].back * g.dz; }
            const double e_out = out[0].e;
            const double e_abs = SPLIT ? e - (two ? out[0].e + out[1].e : out[0].e) : e - e_out;
            unsigned long long hslot = ~0ull;
            record_hit<LDS, CHART>(L, l_tally, s, e, e_abs, hx, hy, hz, g.dx, g.dy, g.dz, P.capture != 0, prev, &hc, l_fm, volume, true, &hslot);
            if (!volume) { ts = s; tea = e_abs; tei = e; }
            if (nW && C.hit_x && hslot != ~0ull) {        // a captured hit of a polychromatic ray: wavelengths, spectrum in, spectrum out
                const double *tab = L.extra + trc_rec_extra_off(rec);
                for (int w = 0; w < nW; ++w) {
                    const double xw = wl_of(w), yin = spec_of(w);
                    const double f = poly_th >= 0.0 ? 1.0 - poly_abs(tab, poly_th, w, xw) : (two ? out[0].sf + out[1].sf : out[0].sf);
                    C.hit_x[(long long)w * C.hit_x_cap + (long long)hslot] = xw;
                    C.hit_x[(long long)(nW + w) * C.hit_x_cap + (long long)hslot] = yin;
                    C.hit_x[(long long)(2 * nW + w) * C.hit_x_cap + (long long)hslot] = yin * f;
                    if (POLY && poly_th >= 0.0) C.slot_spec[(long long)w * W.room + slot] = yin * f;      // (in place: sample w is not read again)
                }
                if (POLY && poly_th >= 0.0) p_done = true;
            }
            if constexpr (SPLIT) {
                // the second ray, before the first goes back into the hit's slot (whose spectrum row it reads)
                const bool on1 = two && out[1].e > P.min_energy;
                if (on1 && bounce0 + 1 >= P.reps) {
                    atomicAdd(&sc.counters[3], 1ull);
                    atomicAdd(sc.energy_left, out[1].e);
                    if (P.flags & TRC_TRACE_KEEP_LAST) {
                        const unsigned long long q = atomicAdd(&sc.counters[2], 1ull);
                        if ((long long)q < P.last_cap) {
                            P.lx[q] = hx + out[1].shift * nx; P.ly[q] = hy + out[1].shift * ny; P.lz[q] = hz + out[1].shift * nz;
                            P.ldx[q] = out[1].dx; P.ldy[q] = out[1].dy; P.ldz[q] = out[1].dz; P.le[q] = out[1].e;
                            if constexpr (POLY) {
                                if (C.last_spec) for (int w = 0; w < nW; ++w) C.last_spec[(long long)w * P.last_cap + (long long)q] = spec_of(w) * out[1].sf;
                                if (C.last_wl) for (int w = 0; w < nW; ++w) C.last_wl[(long long)w * P.last_cap + (long long)q] = wl_of(w);
                            }
                        }
                    }
                }
                alive1 = on1 && bounce0 + 1 < P.reps;
                // (the lanes with a hit are all here: cs is handed to the others behind the region, as the hit buffer's chunk is)
                const unsigned long long sl = chunk_append(&W.cnt[CN(CW_SLOTS)], cs, alive1, nullptr, 0);
                if (alive1 && (long long)sl >= W.room) { W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; alive1 = false; }
                if (alive1) {
                    slot1 = (uint32_t)sl;
                    SRayGeo go;
                    go.px = hx + out[1].shift * nx; go.py = hy + out[1].shift * ny; go.pz = hz + out[1].shift * nz;
                    go.dx = out[1].dx; go.dy = out[1].dy; go.dz = out[1].dz;
                    go.head = SQ_INVALID;
                    go.idx = g.idx;             // (still the place of the bundle's columns: materials, sample wavelengths)
                    uint32_t pw = volume ? (uint32_t)prev : (uint32_t)s;
                    if (!volume && out[1].shift == 0.0 && leaves_flat(rec, hx, hy, hz, out[1].dx, out[1].dy, out[1].dz)) pw |= SQ_SKIP_SELF;
                    go.tail = sray_tail(bounce0 + 1, pw);
                    W.geo[slot1] = go;
                    SRayAux ao;
                    ao.e = out[1].e; ao.ref = out[1].ref; ao.wl = wl; ao.pad = out_im[1];
                    W.aux[slot1] = ao;
                    C.slot_rid[slot1] = trc_child_rid(rid, (uint32_t)(bounce0 + 1));
                    for (int w = 0; w < nW; ++w) C.slot_spec[(long long)w * W.room + slot1] = spec_of(w) * out[1].sf;
                }
            }
            const double ox = out[0].dx, oy = out[0].dy, oz = out[0].dz;
            if (e_out > P.min_energy) {                               // tracer_engine.py:242
                if (bounce0 + 1 >= P.reps) {
                    atomicAdd(&sc.counters[3], 1ull);
                    atomicAdd(sc.energy_left, e_out);
                    if (P.flags & TRC_TRACE_KEEP_LAST) {
                        const unsigned long long q = atomicAdd(&sc.counters[2], 1ull);
                        if ((long long)q < P.last_cap) {
                            P.lx[q] = hx + out[0].shift * nx; P.ly[q] = hy + out[0].shift * ny; P.lz[q] = hz + out[0].shift * nz;
                            P.ldx[q] = ox; P.ldy[q] = oy; P.ldz[q] = oz; P.le[q] = e_out;
                            if constexpr (POLY) {
                                // the spectrum that leaves: at a polychromatic wall the one written above, or evaluated here
                                const double *tab = L.extra + trc_rec_extra_off(rec);
                                if (C.last_spec)
                                    for (int w = 0; w < nW; ++w)
                                        C.last_spec[(long long)w * P.last_cap + (long long)q] =
                                            p_done ? C.slot_spec[(long long)w * W.room + slot]
                                                   : spec_of(w) * (poly_th >= 0.0 ? 1.0 - poly_abs(tab, poly_th, w, wl_of(w)) : out[0].sf);
                                if (C.last_wl) for (int w = 0; w < nW; ++w) C.last_wl[(long long)w * P.last_cap + (long long)q] = wl_of(w);
                            }
                        }
                    }
                } else {
                    alive = true;
                    SRayGeo go;
                    go.px = hx + out[0].shift * nx; go.py = hy + out[0].shift * ny; go.pz = hz + out[0].shift * nz;
                    go.dx = ox; go.dy = oy; go.dz = oz;
                    go.head = SQ_INVALID;
                    go.idx = g.idx;
                    uint32_t pw = volume ? (uint32_t)prev : (uint32_t)s;        // the surface the ray leaves (a volume event: still the one before)
                    if (!volume && out[0].shift == 0.0 && leaves_flat(rec, hx, hy, hz, ox, oy, oz)) pw |= SQ_SKIP_SELF;
                    go.tail = sray_tail(bounce0 + 1, pw);
                    W.geo[slot] = go;
                    SRayAux ao;
                    ao.e = e_out; ao.ref = out[0].ref; ao.wl = wl; ao.pad = out_im[0];
                    W.aux[slot] = ao;
                    if (SPLIT) C.slot_rid[slot] = rid;          // (the first ray keeps the parent's stream)
                    if (nW && !(POLY && p_done)) {       // the spectrum goes on with the ray (RayBundle.inherit, ray_bundle.py:117-143), the optics' changes applied
                        const double *tab = L.extra + trc_rec_extra_off(rec);
                        for (int w = 0; w < nW; ++w) {
                            const double f = poly_th >= 0.0 ? 1.0 - poly_abs(tab, poly_th, w, wl_of(w)) : out[0].sf;
                            C.slot_spec[(long long)w * W.room + slot] = spec_of(w) * f;
                        }
                    }
                }
            }
        }
        tally_by_wave<6>(LDS ? l_tally : L.tally, Sn, ts, tea, tei, (!LDS || Sn <= 64) ? 8 : 0);     // (the loop of k_s_shade_c)
        if (P.capture) chunk_rebroadcast(hc, __ffsll((long long)my_lanes) - 1);
        if (SPLIT) chunk_rebroadcast(cs, __ffsll((long long)my_lanes) - 1);
        const unsigned long long q = chunk_append(&W.cnt[CN(CW_ACT_OUT)], ca, alive, S.act_out, W.act_room);
        if (alive) { if ((long long)q < W.act_room) S.act_out[q] = slot; else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; n_alive += 1; }
        if constexpr (SPLIT) {      // (a wave whose 64 lanes all split appends 128 entries in this turn: a round of its own, so that each fits a chunk)
            const unsigned long long q1 = chunk_append(&W.cnt[CN(CW_ACT_OUT)], ca, alive1, S.act_out, W.act_room);
            if (alive1) { if ((long long)q1 < W.act_room) S.act_out[q1] = slot1; else W.cnt[CN(CW_OVERFLOW)] = CW_OVF_FAIL; n_alive += 1; }
        }
    }
    chunk_close(ca, S.act_out, W.act_room);
    if (P.capture && wave_g < SHADE_MAX_WAVES && lane_id() == 0) hit_chunk_suspend(hc, W.hit_state + 2 * wave_g, S.hit_epoch);
    flush_counts<true>(l_tally + (LDS ? 3 * Sn : 0), n_hit, n_alive, &W.cnt[CN(CW_HITS)], &W.cnt[CN(CW_CLS_HITS + TRC_CLS_GENERAL)], &W.cnt[CN(CW_ALIVE)]);
    flush_sums(L.tally, l_tally, LDS ? 3 * Sn : 0, l_fm, S.lds_fm_bins, Sn);
}

template <bool LDS, bool CHART = false, bool SPLIT = false, bool MAT = false>
__global__ __launch_bounds__(SHC_THREADS) void k_s_shade_x(StreamParams S) { shade_x_body<LDS, CHART, SPLIT, MAT, false>(S); }

// (no MAT x POLY instance: a carried ray has no single wavelength to evaluate m(lambda) at)
template <bool LDS, bool CHART, bool SPLIT>
__global__ __launch_bounds__(SHC_THREADS) void k_s_shade_p(StreamParams S) { shade_x_body<LDS, CHART, SPLIT, false, true>(S); }

const void *trc_shade_poly_kernel(bool lds, bool chart, bool split) {
    if (split) {
        if (chart) return lds ? (const void *)k_s_shade_p<true, true, true> : (const void *)k_s_shade_p<false, true, true>;
        return lds ? (const void *)k_s_shade_p<true, false, true> : (const void *)k_s_shade_p<false, false, true>;
    }
    if (chart) return lds ? (const void *)k_s_shade_p<true, true, false> : (const void *)k_s_shade_p<false, true, false>;
    return lds ? (const void *)k_s_shade_p<true, false, false> : (const void *)k_s_shade_p<false, false, false>;
}

const void *trc_shade_carry_kernel(bool lds, bool chart, bool split, bool mat) {
    if (mat) {      // (no CHART x MAT instance: stream_form_shade never asks for one)
        if (chart) return nullptr;
        if (split) return lds ? (const void *)k_s_shade_x<true, false, true, true> : (const void *)k_s_shade_x<false, false, true, true>;
        return lds ? (const void *)k_s_shade_x<true, false, false, true> : (const void *)k_s_shade_x<false, false, false, true>;
    }
    if (split) {
        if (chart) return lds ? (const void *)k_s_shade_x<true, true, true> : (const void *)k_s_shade_x<false, true, true>;
        return lds ? (const void *)k_s_shade_x<true, false, true> : (const void *)k_s_shade_x<false, false, true>;
    }
    if (chart) return lds ? (const void *)k_s_shade_x<true, true> : (const void *)k_s_shade_x<false, true>;
    return lds ? (const void *)k_s_shade_x<true> : (const void *)k_s_shade_x<false>;
}

const void *trc_shade_lean_kernel(int cls, bool flat, bool lds, bool spec, bool chart) {
    // a scene with a flux map in another chart than XY: the instances for any geometry (such a map lies on a cylinder, a dish or a
    // sphere more often than on a round plate), which serve flat surfaces with the same arithmetic
#define SHC_PICK_CHART(C) (spec ? (lds ? (const void *)k_s_shade_c<C, false, true, true, true> : (const void *)k_s_shade_c<C, false, false, true, true>) \
                                : (lds ? (const void *)k_s_shade_c<C, false, true, false, true> : (const void *)k_s_shade_c<C, false, false, false, true>))
    if (chart && cls == TRC_CLS_MIRROR) return SHC_PICK_CHART(TRC_CLS_MIRROR);
    if (chart && cls == TRC_CLS_DIFFUSE) return SHC_PICK_CHART(TRC_CLS_DIFFUSE);
#undef SHC_PICK_CHART
#define SHC_PICK(C) (spec ? (flat ? (lds ? (const void *)k_s_shade_c<C, true, true, true> : (const void *)k_s_shade_c<C, true, false, true>) \
                                  : (lds ? (const void *)k_s_shade_c<C, false, true, true> : (const void *)k_s_shade_c<C, false, false, true>)) \
                          : (flat ? (lds ? (const void *)k_s_shade_c<C, true, true> : (const void *)k_s_shade_c<C, true, false>) \
                                  : (lds ? (const void *)k_s_shade_c<C, false, true> : (const void *)k_s_shade_c<C, false, false>)))
    if (cls == TRC_CLS_MIRROR) return SHC_PICK(TRC_CLS_MIRROR);
    if (cls == TRC_CLS_DIFFUSE) return SHC_PICK(TRC_CLS_DIFFUSE);
#undef SHC_PICK
    return nullptr;
}
