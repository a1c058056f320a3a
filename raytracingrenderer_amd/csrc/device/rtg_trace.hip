// rtg_trace.hip — the traversal of the wavefront renderers: k_trace (closest-hit and any-hit rays in
// one persistent launch), its launch and grid sizing, the ray queries of include/rtg.h, and the
// RTG_DEBUG capture + replay of its record fetches. rtg_render.hip's header describes the loop that
// launches it; rtg_scene.hip builds the trees it walks.
#include "rtg_internal.h"

#include <algorithm>

// ------------------------------------------------------------------ traversal
// Persistent lanes with per-lane ray replacement: a wave takes 64 ray indices at a time from the
// queue (one atomic per 64 rays) into a wave-uniform pool, and every lane whose ray terminates
// immediately takes the next index from the pool. Without replacement a wave runs until its
// longest ray finishes (measured SIMD efficiency ~27 %).
// Work slice k of a trace launch. Path tracer (segmented queues, io.seg_cap != 0; io.fetch8: one
// counter per slice, by blockIdx % 8, i.e. one per XCD): slice k is queue segment k, its extension
// rays at positions [k * seg_cap, + elen) and then its shadow rays at the same shadow positions, so
// every XCD walks long closest-hit rays first and ends on any-hit rays; len rays in all. Otherwise
// (one counter: light tracer, ray queries): every ray, extension rays first.
static __device__ __forceinline__ void trace_slice(const TraceIO& io, unsigned nc, unsigned n, int k, unsigned& elo,
                                                   unsigned& elen, unsigned& len) {
    if (io.seg_cap) {
        elo = (unsigned)k * io.seg_cap;
        elen = io.seg_ne ? io.seg_ne[32 * k] : 0u;
        len = elen + (io.seg_ns ? io.seg_ns[32 * k] : 0u);
    } else {
        elo = 0;
        elen = nc;
        len = n;
    }
}

// SMALL: the scene's wide nodes, triangle records and leaf boxes are copied into LDS at the start of
// each block (SceneView::img, small scenes only) and the walk reads them there; the LDS stack is then
// RTG_STACK_SMALL entries, so the block's LDS stays below 5 KB (7 one-wave blocks per SIMD, as the
// global walk's 16-entry stack).
template <bool COUNT, bool SMALL>
__global__ __launch_bounds__(RTG_TTB) __attribute__((amdgpu_waves_per_eu(RTG_TRACE_WPE)))
void k_trace(SceneView s, TraceIO io) {
    constexpr int STK = SMALL ? RTG_STACK_SMALL : RTG_STACK;
    __shared__ int stk[STK][RTG_TTB];
    __shared__ float kstk[COUNT ? STK : 1][RTG_TTB];  // COUNT only: entry key of each push
    __shared__ float4 s_img[SMALL ? RTG_SMALL_F4 : 1];
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const unsigned gthreads = gridDim.x * blockDim.x;
    const unsigned gtid = blockIdx.x * blockDim.x + tid;
    // extension index span: the ray count, or (segmented queues) all 8 segments' positions
    const unsigned nc = io.seg_cap ? 8u * io.seg_cap : (io.count ? *io.count : 0u);
    const unsigned n = nc + (io.scount ? *io.scount : 0u);
    unsigned long long c_nodes = 0, c_tris = 0, c_snodes = 0, c_stris = 0, c_slots = 0, c_nstep = 0, c_lstep = 0,
                       c_cullpop = 0, c_pops = 0, c_lslots = 0, c_lbox = 0;
    unsigned c_tails = 0;  // triangle records whose last 16 B were fetched (COUNT)
    // COUNT: why a lane is not stepping a node in an iteration: no ray, its walk done but its parked
    // leaf not run yet, a leaf reached while both parked-leaf slots are full, retiring this iteration, a leaf
    // popped last iteration (parked in this one)
    unsigned long long c_idle_e = 0, c_idle_ll = 0, c_idle_lb = 0, c_idle_r = 0, c_idle_lp = 0;
    unsigned pool_base = 0, pool_left = 0, last_b = 0;  // wave-uniform
    const unsigned tail_rays = (gthreads / 64u) * (unsigned)RTG_FETCH * RTG_FETCH_TAIL / (io.fetch8 ? 8u : 1u);
    // the 8 slices (trace_slice) in LDS, read when a wave fetches work: the loop keeps only the
    // slice number in a register
    __shared__ unsigned s_tab[3][8];
    if (tid < 8) {
        unsigned elo, elen, len;
        trace_slice(io, nc, n, tid, elo, elen, len);
        s_tab[0][tid] = elo;
        s_tab[1][tid] = elen;
        s_tab[2][tid] = len;
        // the host's next k_shade grid (TraceIO::hcnt): a volatile vector store, emitted with the
        // system-scope bits (sc0 sc1). (__hip_atomic_store at system scope cost the walk 4 VGPR spills)
        if (io.hcnt && blockIdx.x == 0) ((volatile unsigned*)io.hcnt)[tid] = elen;
    }
    if (SMALL)
        for (int i = tid; i < s.img_n4; i += RTG_TTB) s_img[i] = s.img[i];
    __syncthreads();
    const DevTri48* tris = SMALL ? reinterpret_cast<const DevTri48*>(s_img + s.img_tri) : s.tris48;
    // (the leaf boxes stay in global memory, read once per candidate hit: with them the image of
    // the cornell box would not fit RTG_SMALL_F4)
    const float4* lboxes = s.leafbox;
    int slice = io.fetch8 ? (int)(blockIdx.x & 7u) : 0, tried = 0;  // wave-uniform
    unsigned s_len = __builtin_amdgcn_readfirstlane(s_tab[2][slice]);
    bool drained = false;                   // wave-uniform
    bool have = false;
    unsigned ri = 0;
    v3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tbest = 0.0f, omag = 0.0f, dmag = 0.0f, delta = 0.0f, bu = 0.0f, bv = 0.0f;
    int bid = -1, pid = 0, cur = RTG_EXIT, sp = 0, pend = RTG_EXIT;
    int pend2 = RTG_EXIT;  // a second parked leaf (the leaf phase runs pend, then pend2 moves up)
    bool occluded = false, wide = false, anyr = false;  // anyr: this lane's ray is a shadow ray
    const unsigned wslot = gtid >> 6;
    // RTG_DEBUG capture: the ray's record fetches in order (cap_k of them so far)
    unsigned cap_ri = 0, cap_k = 0;
    uint4 cap_q = make_uint4(0, 0, 0, 0);
    auto capture = [&](unsigned type, unsigned idx) {
        if (!RTG_DEBUG || !io.cap) return;
        if (cap_k < RTG_CAP_LEN) {
            const unsigned e = (type << 30) | idx;
            const unsigned j = cap_k & 3;
            cap_q.x = j == 0 ? e : cap_q.x;
            cap_q.y = j == 1 ? e : cap_q.y;
            cap_q.z = j == 2 ? e : cap_q.z;
            cap_q.w = j == 3 ? e : cap_q.w;
            if (j == 3) io.cap[(size_t)(cap_k >> 2) * io.cap_n + cap_ri] = cap_q;
        }
        ++cap_k;
    };
    if (RTG_DEBUG && io.wtime && lane == 0) io.wtime[3 * wslot] = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        // ---- retire finished rays
        if (have && cur == RTG_EXIT && pend == RTG_EXIT && pend2 == RTG_EXIT) {
            if (anyr) {
                if (io.visible) io.visible[pid] = occluded ? 0 : 1;
                else if (bid == -2 ? occluded : !occluded)
                    io.contrib[pid] = bid == -2 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : io.sray_c[pid];
            } else {
                io.hits[pid] = make_float4(tbest, __int_as_float(bid), bu, bv);
            }
            if (RTG_DEBUG && io.cap) {
                const unsigned k = min(cap_k, (unsigned)RTG_CAP_LEN);
                if (k & 3) io.cap[(size_t)(k >> 2) * io.cap_n + cap_ri] = cap_q;
                io.cap_len[cap_ri] = cap_k;  // the true count; the first RTG_CAP_LEN are kept
            }
            have = false;
        }
        // ---- refill idle lanes from the wave's pool
        const unsigned long long im = __ballot(!have);
        if (im != 0 && !drained && (__popcll(im) >= RTG_REFILL || __ballot(have) == 0)) {
            // wave-uniform fetch: big batches (one atomic per fetch_big rays) until about
            // RTG_FETCH_TAIL rounds of them are left in the slice, judged from this wave's previous
            // fetch, then 64 (shorter drain tails). With io.fetch8 the index space is cut into 8
            // slices with a counter each (the atomics of one counter serialise); a wave starts on
            // slice blockIdx % 8 and moves on to the next slice when its own runs dry.
            while (pool_left == 0) {
                const bool tail = last_b + tail_rays >= s_len;
                const unsigned g = tail ? (unsigned)RTG_TAIL_BATCH : (unsigned)RTG_FETCH;
                unsigned b = 0;
                if (lane == 0) b = atomicAdd(io.fetch8 ? io.fetch8 + 32 * slice : io.fetch, g);
                b = __builtin_amdgcn_readfirstlane(b);  // wave-uniform: keeps the fetch state in SGPRs
                last_b = b;
                if (b < s_len) {
                    pool_base = b;
                    pool_left = min(g, s_len - b);
                } else if (!io.fetch8 || ++tried == 8) {
                    drained = true;
                    if (RTG_DEBUG && io.wtime && lane == 0) io.wtime[3 * wslot + 1] = __builtin_amdgcn_s_memrealtime();
                    break;
                } else {
                    slice = (slice + 1) & 7;
                    s_len = __builtin_amdgcn_readfirstlane(s_tab[2][slice]);
                    last_b = s_len;  // a stolen slice is near its end: small batches
                }
            }
            if (pool_left > 0) {
                const unsigned pos = prefix_lt(im);
                const unsigned take = min((unsigned)__popcll(im), pool_left);
                if (!have && pos < take) {
                    const unsigned j = pool_base + pos;  // index within the slice
                    const unsigned s_elo = s_tab[0][slice], s_elen = s_tab[1][slice];
                    ri = j < s_elen ? s_elo + j : nc + s_elo + (j - s_elen);
                    have = true;
                    if (RTG_DEBUG) { cap_ri = ri; cap_k = 0; }
                    anyr = ri >= nc;
                    pid = (int)(anyr ? io.squeue[ri - nc] : (io.queue ? io.queue[ri] : ri));
                    // io.spos: the shadow ray sits at its shadow-queue position (no dependence on the
                    // id load; the id is needed when the ray retires)
                    const unsigned sk = io.spos ? ri - nc : (unsigned)pid;
                    const float4 ro = anyr ? io.sray_o[sk] : (io.ray_o ? io.ray_o[pid] : io.cam_o);
                    const float4 rd = anyr ? io.sray_d[sk] : io.ray_d[pid];
                    // sh_d.w != 0: the shadow value is in sray_c and is copied on visibility;
                    // 0: k_shade already stored it in contrib, which is cleared on occlusion
                    // (kept in bid, which a shadow ray does not use: -2 = value already in contrib)
                    o = mk(ro.x, ro.y, ro.z);
                    d = mk(rd.x, rd.y, rd.z);
                    tbest = anyr ? ro.w : RTG_FLT_MAX;
                    inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // Ray::init
                    omag = s.cull_scale + fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
                    dmag = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
                    delta = RTG_CULL_REL * (omag + (tbest < RTG_FLT_MAX ? tbest * dmag : 0.0f));
                    bid = (anyr && !io.visible && rd.w == 0.0f) ? -2 : -1;
                    bu = bv = 0.0f;
                    occluded = false;
                    sp = 0;
                    pend = RTG_EXIT;
                    pend2 = RTG_EXIT;
                    // Wide walk only when every 1/d component is finite and nonzero (no NaN slab
                    // terms): then a passing descendant box implies its skipped ancestors pass.
                    // (|1/d| <= 2^64 and scene scale in [2^-60, 2^60] keep every product of the
                    // compressed walk finite and normal.)
                    wide = io.wide && s.usew && fabsf(inv.x) <= 0x1p64f && fabsf(inv.y) <= 0x1p64f &&
                           fabsf(inv.z) <= 0x1p64f && inv.x != 0.0f && inv.y != 0.0f && inv.z != 0.0f;
                    const float* rb = s.root_box;
                    cur = slab_exact(rb[0], rb[1], rb[2], rb[3], rb[4], rb[5], o, inv)
                              ? (wide ? s.root_wordw : s.root_word) : RTG_EXIT;
                }
                pool_base += take;
                pool_left -= take;
            }
        }
        if (drained && __ballot(have) == 0) break;
        if (COUNT) {
            c_slots += 64;
            c_nstep += (have && cur >= 0) ? 1 : 0;
            c_idle_e += !have ? 1 : 0;
            c_idle_ll += (have && cur == RTG_EXIT && pend != RTG_EXIT) ? 1 : 0;
            c_idle_lb += (have && cur < 0 && cur != RTG_EXIT && pend != RTG_EXIT && pend2 != RTG_EXIT) ? 1 : 0;
            c_idle_r += (have && cur == RTG_EXIT && pend == RTG_EXIT) ? 1 : 0;
            c_idle_lp += (have && cur < 0 && cur != RTG_EXIT && (pend == RTG_EXIT || pend2 == RTG_EXIT)) ? 1 : 0;
        }
        if (!have || (cur == RTG_EXIT && pend == RTG_EXIT && pend2 == RTG_EXIT)) continue;
        // Leaf: the reference's leaf loop (Geometry.h:420-431 / 446-458) over 1-2 triangles (a wide
        // leaf slot may join sibling reference leaves: up to RTG_LEAF_SPAN triangles).
        auto leaf = [&](const int word) {
            const int code = ~word;
            const int start = code / RTG_LEAF_SPAN;  // leaf word ~(start * RTG_LEAF_SPAN + count - 1)
            const int cnt = (code % RTG_LEAF_SPAN) + 1;
            for (int k = 0; k < cnt; ++k) {
                const int tri = start + k;
                if (COUNT) (anyr ? c_stris : c_tris) += 1;
                capture(1u, (unsigned)tri);
                float t, u, v;
                const bool hit = tri_intersect48p(tris + tri, o, d, [&](float tt) {
                    return anyr ? (tt < tbest && tt > RTG_EPS) : (tt <= tbest && tt > RTG_EPS);
                }, t, u, v, c_tails);
                if (hit) {
                    bool cand = anyr ? !(t >= tbest || t <= RTG_EPS)
                                     : (t > RTG_EPS && (t < tbest || (t == tbest && tri < bid)));
                    if (cand && wide) {
                        // the exact box of the reference leaf holding this triangle (stored per
                        // triangle: a wide leaf slot may join sibling reference leaves)
                        const float4 b0 = lboxes[2 * tri], b1 = lboxes[2 * tri + 1];
                        if (COUNT) c_lbox += 1;
                        capture(2u, (unsigned)tri);
                        cand = slab_exact(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, o, inv);
                    }
                    if (!cand) {
                    } else if (anyr) {
                        occluded = true;
                    } else {
                        tbest = t;
                        bid = tri;
                        bu = u;
                        bv = v;
                        delta = RTG_CULL_REL * (omag + tbest * dmag);
                    }
                }
            }
        };
        // ---- one traversal step
        if (cur >= 0 && wide) {
            int wd[4];
            float key[4];
            {
                capture(0u, (unsigned)cur);
                const float4* np = SMALL ? s_img + 4 * cur : s.nodesq[cur].q;
                const float4 h0 = np[0], h1 = np[1], h2 = np[2], h3 = np[3];
                const unsigned ex = __float_as_uint(h0.w);
                const float sx = __uint_as_float((ex & 255u) << 23);
                const float sy = __uint_as_float(((ex >> 8) & 255u) << 23);
                const float sz = __uint_as_float(((ex >> 16) & 255u) << 23);
                const unsigned p0 = __float_as_uint(h1.x), p1 = __float_as_uint(h1.y), p2 = __float_as_uint(h1.z);
                const unsigned p3 = __float_as_uint(h1.w), p4 = __float_as_uint(h2.x), p5 = __float_as_uint(h2.y);
                wd[0] = __float_as_int(h2.z);
                wd[1] = __float_as_int(h2.w);
                wd[2] = __float_as_int(h3.x);
                wd[3] = __float_as_int(h3.y);
                // Conservative slot test in ray-relative form. Exactness does not need the exact slab
                // test here: a candidate hit is accepted only after its reference leaf box passes the
                // exact test, so a slot test only has to pass whenever the exact test on a reference
                // box inside the slot passes. Per axis, with s the power-of-two step:
                //   near entry  tn = fma(q_near, s*inv, ((origin + mn) - o) * inv)
                //   far exit    tf = fma(q_far,  s*inv, ((origin - mn) - o) * inv)
                // mn moves the near plane (and -mn the far plane) outward by mu = 2^-16 (scale + |o|).
                // The rounding of this form plus the reference's own is below 2^-19.5 (scale + |o|)|inv|
                // per plane, inside the mu |inv| margin, so tn <= the reference entry
                // and tf >= the reference exit of every box the slot contains.
                // Cull key: max(tn) - (delta - mu) * max|inv| is below the entry of the slot's box
                // inflated by delta (slab_cull_entry's conservative bound).
                const bool px = inv.x > 0.0f, py = inv.y > 0.0f, pz = inv.z > 0.0f;
                const unsigned nqx = px ? p0 : p3, fqx = px ? p3 : p0;
                const unsigned nqy = py ? p1 : p4, fqy = py ? p4 : p1;
                const unsigned nqz = pz ? p2 : p5, fqz = pz ? p5 : p2;
                const float mu = RTG_CULL_REL * omag;
                const float mnx = px ? -mu : mu, mny = py ? -mu : mu, mnz = pz ? -mu : mu;
                // packed FP32 (v_pk_*): per-component IEEE results identical to the scalar ops
                const f2 ax2 = ((f2){h0.x, h0.x} + (f2){mnx, -mnx} - (f2){o.x, o.x}) * (f2){inv.x, inv.x};
                const f2 ay2 = ((f2){h0.y, h0.y} + (f2){mny, -mny} - (f2){o.y, o.y}) * (f2){inv.y, inv.y};
                const f2 az2 = ((f2){h0.z, h0.z} + (f2){mnz, -mnz} - (f2){o.z, o.z}) * (f2){inv.z, inv.z};
                const float six = sx * inv.x, siy = sy * inv.y, siz = sz * inv.z;
                const f2 six2 = {six, six}, siy2 = {siy, siy}, siz2 = {siz, siz};
                const f2 anx2 = {ax2.x, ax2.x}, afx2 = {ax2.y, ax2.y};
                const f2 any2 = {ay2.x, ay2.x}, afy2 = {ay2.y, ay2.y};
                const f2 anz2 = {az2.x, az2.x}, afz2 = {az2.y, az2.y};
                const float cshift = (delta - mu) * fmaxf(fmaxf(fabsf(inv.x), fabsf(inv.y)), fabsf(inv.z));
#pragma unroll
                for (int k = 0; k < 4; k += 2) {  // slot pairs (k, k+1)
                    auto q2 = [&](unsigned plane) {
                        return (f2){(float)((plane >> (8 * k)) & 255u), (float)((plane >> (8 * k + 8)) & 255u)};
                    };
                    const f2 tnx = __builtin_elementwise_fma(q2(nqx), six2, anx2);
                    const f2 tny = __builtin_elementwise_fma(q2(nqy), siy2, any2);
                    const f2 tnz = __builtin_elementwise_fma(q2(nqz), siz2, anz2);
                    const f2 tfx = __builtin_elementwise_fma(q2(fqx), six2, afx2);
                    const f2 tfy = __builtin_elementwise_fma(q2(fqy), siy2, afy2);
                    const f2 tfz = __builtin_elementwise_fma(q2(fqz), siz2, afz2);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float en = fmaxf(fmaxf(tnx[j], tny[j]), tnz[j]);
                        const float tx = fminf(fminf(tfx[j], tfy[j]), tfz[j]);
                        const float e = en - cshift;
                        // (finite here, so a miss is the only +inf key)
                        // (bitwise & / |: no branches per slot)
                        const bool hit = (wd[k + j] != RTG_EXIT) & !((tx < en) | (tx < 0.0f)) & (!io.cull | !(e > tbest));
                        if (COUNT) (anyr ? c_snodes : c_nodes) += wd[k + j] != RTG_EXIT ? 1 : 0;
                        key[k + j] = hit ? e : __builtin_inff();
                    }
                }
            }
            // ascending entry distance (misses sort last); order only affects culling, not results
#define RTG_CSWAP(i, j)                                               \
    if (key[j] < key[i]) {                                           \
        const float tk = key[i]; key[i] = key[j]; key[j] = tk;      \
        const int tw = wd[i]; wd[i] = wd[j]; wd[j] = tw;             \
    }
            RTG_CSWAP(0, 1) RTG_CSWAP(2, 3) RTG_CSWAP(0, 2) RTG_CSWAP(1, 3) RTG_CSWAP(1, 2)
#undef RTG_CSWAP
            // misses carry +inf and sort last
            if (key[0] == __builtin_inff()) {
                cur = RTG_POP;
            } else if (!COUNT && sp + 3 <= STK) {
                // hits are a prefix of the sorted slots: push the h = hits - 1 far ones (far first)
                // with three unconditional LDS writes; entries above sp + h are never read
                const int h = (key[1] != __builtin_inff()) + (key[2] != __builtin_inff()) + (key[3] != __builtin_inff());
                stk[sp][tid] = h == 3 ? wd[3] : (h == 2 ? wd[2] : wd[1]);
                stk[sp + 1][tid] = h == 3 ? wd[2] : wd[1];
                stk[sp + 2][tid] = wd[1];
                sp += h;
                cur = wd[0];
            } else {
#pragma unroll
                for (int k = 3; k >= 1; --k) {
                    if (key[k] != __builtin_inff()) {
                        if (COUNT && sp < STK) kstk[sp][tid] = key[k];
                        if (sp < STK) stk[sp][tid] = wd[k];
                        else io.ovf[(size_t)(sp - STK) * gthreads + gtid] = wd[k];
                        ++sp;
                    }
                }
                cur = wd[0];
            }
        } else if (cur >= 0) {
            if (COUNT) (anyr ? c_snodes : c_nodes) += 2;
            capture(3u, (unsigned)cur);
            const DevNode nd = s.nodes[cur];
            bool hl = slab_exact(nd.a.x, nd.a.y, nd.a.z, nd.a.w, nd.b.x, nd.b.y, o, inv);
            bool hr = slab_exact(nd.b.z, nd.b.w, nd.c.x, nd.c.y, nd.c.z, nd.c.w, o, inv);
            const float el = slab_cull_entry(nd.a.x, nd.a.y, nd.a.z, nd.a.w, nd.b.x, nd.b.y, o, inv, delta);
            const float er = slab_cull_entry(nd.b.z, nd.b.w, nd.c.x, nd.c.y, nd.c.z, nd.c.w, o, inv, delta);
            if (io.cull) {
                hl = hl && !(el > tbest);
                hr = hr && !(er > tbest);
            }
            if (hl && hr) {
                const bool lfirst = !(er < el);
                const int nearw = lfirst ? nd.d.x : nd.d.y;
                const int farw = lfirst ? nd.d.y : nd.d.x;
                if (COUNT && sp < STK) kstk[sp][tid] = -RTG_FLT_MAX;
                if (sp < STK) stk[sp][tid] = farw;
                else io.ovf[(size_t)(sp - STK) * gthreads + gtid] = farw;
                ++sp;
                cur = nearw;
            } else if (hl) {
                cur = nd.d.x;
            } else if (hr) {
                cur = nd.d.y;
            } else {
                cur = RTG_POP;
            }
        }
        // park a reached leaf and keep walking; a second one instead of idling until the leaf phase
        // (node-step lane use 0.70 -> 0.77 on C3)
        if (cur < 0 && cur != RTG_EXIT && cur != RTG_POP && pend == RTG_EXIT) {
            pend = cur;
            cur = RTG_POP;
        } else if (cur < 0 && cur != RTG_EXIT && cur != RTG_POP && pend2 == RTG_EXIT) {
            pend2 = cur;
            cur = RTG_POP;
        }
        // ---- one pop for every branch: always an LDS read (ds_read, not a flat load through a
        // selected pointer); the global overflow read only for deep entries
        if (cur == RTG_POP) {
            if (COUNT && !anyr && sp > 0) c_pops += 1;
            if (sp == 0) {
                cur = RTG_EXIT;
            } else {
                --sp;
                cur = stk[sp < STK ? sp : 0][tid];
                if (COUNT && !anyr && sp < STK && kstk[sp][tid] > tbest) c_cullpop += 1;
                if (sp >= STK) cur = io.ovf[(size_t)(sp - STK) * gthreads + gtid];
            }
        }
        // leaf phase (wave-uniform): enough parked leaves, or no lane can walk on, or (the queue is
        // dry) any parked leaf: the drain is latency-bound, lanes should not wait for each other
        const unsigned long long pm = __ballot(pend != RTG_EXIT);
        if (__popcll(pm) >= RTG_POSTPONE || __ballot(cur >= 0) == 0 || (drained && pm)) {
            if (COUNT) {
                c_lslots += 64;
                c_lstep += pend != RTG_EXIT ? 1 : 0;
            }
            if (pend != RTG_EXIT) {
                leaf(pend);
                pend = pend2;
                pend2 = RTG_EXIT;
                if (anyr && occluded) {
                    cur = RTG_EXIT;
                    sp = 0;
                    pend = RTG_EXIT;
                }
            }
        }
    }
    if (RTG_DEBUG && io.wtime && lane == 0) io.wtime[3 * wslot + 2] = __builtin_amdgcn_s_memrealtime();
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1) {
            c_nodes += __shfl_down(c_nodes, off);
            c_tris += __shfl_down(c_tris, off);
            c_snodes += __shfl_down(c_snodes, off);
            c_stris += __shfl_down(c_stris, off);
            c_nstep += __shfl_down(c_nstep, off);
            c_lstep += __shfl_down(c_lstep, off);
            c_cullpop += __shfl_down(c_cullpop, off);
            c_pops += __shfl_down(c_pops, off);
            c_lbox += __shfl_down(c_lbox, off);
            c_tails += __shfl_down(c_tails, off);
            c_idle_e += __shfl_down(c_idle_e, off);
            c_idle_ll += __shfl_down(c_idle_ll, off);
            c_idle_lb += __shfl_down(c_idle_lb, off);
            c_idle_r += __shfl_down(c_idle_r, off);
            c_idle_lp += __shfl_down(c_idle_lp, off);
        }
        if (lane == 0) {
            atomicAdd(&io.stats[0], c_nodes);
            atomicAdd(&io.stats[1], c_tris);
            atomicAdd(&io.stats[4], c_snodes);
            atomicAdd(&io.stats[5], c_stris);
            atomicAdd(&io.stats[8], c_slots);
            atomicAdd(&io.stats[9], c_nstep);
            atomicAdd(&io.stats[10], c_lstep);
            atomicAdd(&io.stats[13], c_lslots);
            atomicAdd(&io.stats[11], c_cullpop);
            atomicAdd(&io.stats[12], c_pops);
            atomicAdd(&io.stats[6], (unsigned long long)c_tails);
            atomicAdd(&io.stats[7], c_lbox);
            atomicAdd(&io.stats[15], c_idle_e);
            atomicAdd(&io.stats[16], c_idle_ll);
            atomicAdd(&io.stats[17], c_idle_lb);
            atomicAdd(&io.stats[18], c_idle_r);
            atomicAdd(&io.stats[19], c_idle_lp);
        }
    }
}

// The slice table of the captured launch (trace_slice for k = 0..7: elo, elen, slo, shadow count at
// [k], [8 + k], [16 + k], [24 + k]; [32] the extension index span, [33] / [34] the ray counts).
__global__ void k_cap_slices(TraceIO io, unsigned* tab) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned nc = io.seg_cap ? 8u * io.seg_cap : (io.count ? *io.count : 0u);
    const unsigned n = nc + (io.scount ? *io.scount : 0u);
    unsigned te = 0, ts = 0;
    for (int k = 0; k < 8; ++k) {
        unsigned elo, elen, len;
        trace_slice(io, nc, n, k, elo, elen, len);
        if (!io.fetch8 && k > 0) elo = elen = len = 0;  // one work counter: a single slice (slice 0)
        tab[k] = elo;
        tab[8 + k] = elen;
        tab[16 + k] = elo;
        tab[24 + k] = len - elen;
        te += elen;
        ts += len - elen;
    }
    tab[32] = nc;
    tab[33] = te;
    tab[34] = ts;
}

#if RTG_DEBUG
// ------------------------------------------------------------------ locality-matched ceiling
// Replays the record fetches k_trace made for every ray of one launch (captured in order by
// RTG_OPT_CAPTURE) on the scene's own arrays: the same record types, addresses, per-ray order and
// ray-to-lane grouping, with nothing else in the loop but the fetch of the next chain entry (one
// coalesced uint4 per four steps) and 64 dependent VALU per step, at k_trace's occupancy and with
// its work distribution (8 slice counters by blockIdx % 8, 64-ray pool batches, per-lane refill).
// Each fetch's address depends on the previous record's data (xor with `zero` = 0 at run time), so
// every ray is one dependent chain, as in the walk. Its time is the memory system's time for this
// exact access stream: the ceiling k_trace's time is compared against. Between fetches
// a chain of RTG_REPLAY_VALU dependent FMAs (round 4: 64, which the round-5 walk outran: the ceiling
// must hold less work per fetch than the walk does).
#ifndef RTG_REPLAY_VALU
#define RTG_REPLAY_VALU 8
#endif
__global__ __launch_bounds__(RTG_TB) __attribute__((amdgpu_waves_per_eu(RTG_TRACE_WPE)))
void k_replay(SceneView s, const uint4* cap, const unsigned* cap_len, const unsigned* tab, unsigned cap_n,
              unsigned zero, unsigned* fetch8, unsigned long long* total, float* out) {
    const int lane = lane_id();
    const int slice0 = (int)(blockIdx.x & 7u);
    int slice = slice0, tried = 0;
    const unsigned nc = tab[32];
    unsigned s_elo = tab[slice], s_elen = tab[8 + slice], s_slo = tab[16 + slice], s_len = s_elen + tab[24 + slice];
    unsigned pool_base = 0, pool_left = 0;
    bool drained = false, have = false;
    unsigned ri = 0, k = 0, len = 0, dep = 0;
    uint4 q = make_uint4(0, 0, 0, 0);
    float acc = 0.0f;
    unsigned long long fetches = 0;
    for (;;) {
        const unsigned long long im = __ballot(!have);
        if (im != 0 && !drained) {
            while (pool_left == 0) {
                unsigned b = 0;
                if (lane == 0) b = atomicAdd(fetch8 + 32 * slice, 64u);
                b = __builtin_amdgcn_readfirstlane(b);
                if (b < s_len) {
                    pool_base = b;
                    pool_left = min(64u, s_len - b);
                } else if (++tried == 8) {
                    drained = true;
                    break;
                } else {
                    slice = (slice + 1) & 7;
                    s_elo = tab[slice];
                    s_elen = tab[8 + slice];
                    s_slo = tab[16 + slice];
                    s_len = s_elen + tab[24 + slice];
                }
            }
            if (pool_left > 0) {
                const unsigned pos = prefix_lt(im);
                const unsigned take = min((unsigned)__popcll(im), pool_left);
                if (!have && pos < take) {
                    const unsigned j = pool_base + pos;
                    ri = j < s_elen ? s_elo + j : nc + s_slo + (j - s_elen);
                    len = ri < cap_n ? min(cap_len[ri], (unsigned)RTG_CAP_LEN) : 0u;
                    k = 0;
                    have = len > 0;
                }
                pool_base += take;
                pool_left -= take;
            }
        }
        if (drained && __ballot(have) == 0) break;
        if (!have) continue;
        // the chain entries stream past once: non-temporal, so they do not evict the scene's lines
        // from L2 / MALL (with plain loads the replay's 16 B per 4 fetches made it slower than the
        // round-5 walk on C3 and C4)
        if ((k & 3) == 0) {
            typedef unsigned u4v __attribute__((ext_vector_type(4)));
            const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(cap) + (size_t)(k >> 2) * cap_n + ri);
            q = make_uint4(v.x, v.y, v.z, v.w);
        }
        const unsigned j = k & 3;
        const unsigned e = (j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w) ^ (dep & zero);
        const unsigned type = e >> 30, idx = e & 0x3fffffffu;
        float sum;
        if (type == 0) {
            const float4* r = s.nodesq[idx].q;
            const float4 a = r[0], b = r[1], c = r[2], d = r[3];
            sum = (((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w))) + (((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w)));
        } else if (type == 1) {
            const float4 a = s.tris48[idx].a, b = s.tris48[idx].b;  // the head: n and v0 decide t
            sum = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
        } else if (type == 2) {
            const float4 a = s.leafbox[2 * idx], b = s.leafbox[2 * idx + 1];
            sum = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
        } else {
            const DevNode nd = s.nodes[idx];
            sum = (((nd.a.x + nd.a.y) + (nd.a.z + nd.a.w)) + ((nd.b.x + nd.b.y) + (nd.b.z + nd.b.w))) +
                  (((nd.c.x + nd.c.y) + (nd.c.z + nd.c.w)) + __int_as_float(nd.d.x ^ nd.d.y));
        }
#pragma unroll
        for (int v = 0; v < RTG_REPLAY_VALU; ++v) sum = __builtin_fmaf(sum, 1.0000001f, (float)v);
        acc += sum;
        dep = __float_as_uint(sum);
        ++fetches;
        if (++k == len) have = false;
    }
    for (int off = 32; off > 0; off >>= 1) fetches += __shfl_down(fetches, off);
    if (lane == 0) atomicAdd(total, fetches);
    if (acc == 1.2345f) out[0] = acc;  // keep the loads
}
#endif

// ------------------------------------------------------------------ host side
typedef void (*TraceKernel)(SceneView, TraceIO);
static const TraceKernel k_trace_variant[2][2] = {{k_trace<false, false>, k_trace<false, true>},
                                                  {k_trace<true, false>, k_trace<true, true>}};  // [COUNT][SMALL]

// The resident grid of each k_trace variant on h's device (rtg_handle::trace_blocks)
int size_trace_grids(rtg_handle* h) {
    for (int small = 0; small < 2; ++small)
        for (int count = 0; count < 2; ++count) {
            int occ = 0;
            HIPOK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_trace_variant[count][small], RTG_TTB, 0));
            h->trace_blocks[count][small] = h->n_cu * std::max(1, occ);
        }
    return RTG_OK;
}

int launch_trace(rtg_handle* h, const TraceIO& io, hipStream_t st, unsigned max_blocks) {
    const int small = h->sv.img != nullptr, count = h->count != 0;
    const unsigned full = (unsigned)h->trace_blocks[count][small];
    hipLaunchKernelGGL(k_trace_variant[count][small], dim3(max_blocks ? std::min(full, max_blocks) : full),
                       dim3(RTG_TTB), 0, st, h->sv, io);
    LAUNCH_OK("k_trace");
    return RTG_OK;
}

// RTG_DEBUG builds, RTG_OPT_CAPTURE: buffers for the record fetches of the launch `io` describes, its
// slice table (k_cap_slices) on stream ss, and io's capture fields
int capture_begin(rtg_handle* h, TraceIO& io, unsigned seg_tiles, hipStream_t ss) {
    const size_t cn = 2 * (size_t)seg_tiles * 8 * RTG_TB;  // both index spans
    (void)hipFree(h->d_cap);
    (void)hipFree(h->d_cap_len);
    h->d_cap = nullptr;
    h->d_cap_len = nullptr;
    HIPOK(hipMalloc((void**)&h->d_cap, cn * (RTG_CAP_LEN / 4) * sizeof(uint4)));
    HIPOK(hipMalloc((void**)&h->d_cap_len, cn * sizeof(unsigned)));
    if (!h->d_cap_rays) HIPOK(hipMalloc((void**)&h->d_cap_rays, 35 * sizeof(unsigned)));
    HIPOK(hipMemsetAsync(h->d_cap_len, 0, cn * sizeof(unsigned), ss));
    hipLaunchKernelGGL(k_cap_slices, dim3(1), dim3(64), 0, ss, io, h->d_cap_rays);
    LAUNCH_OK("k_cap_slices");
    h->cap_n = (unsigned)cn;
    io.cap = h->d_cap;
    io.cap_len = h->d_cap_len;
    io.cap_n = (unsigned)cn;
    return RTG_OK;
}

static int trace_query(rtg_handle* h, const float* rays, uint32_t n, float* hits, int32_t* vis, bool any) {
    if (!h || !rays || (!hits && !vis)) return RTG_ERR_ARG;
    if (n == 0) return RTG_OK;
    int rc = settle(h);  // slot 0's overflow stack is free
    if (rc) return rc;
    // path-id indirection of the trace kernels: identity queue over n query rays
    DevBuf<float4> d_o, d_d;
    DevBuf<unsigned> d_q;
    DevBuf<char> d_out;
    {
        std::vector<float4> vo(n), vd(n);
        std::vector<unsigned> q(n);
        for (uint32_t i = 0; i < n; ++i) {
            const float* r = rays + (size_t)i * 8;
            vo[i] = make_float4(r[0], r[1], r[2], any ? r[3] : 0.0f);
            vd[i] = make_float4(r[4], r[5], r[6], 0.0f);
            q[i] = i;
        }
        if ((rc = d_o.upload(vo)) || (rc = d_d.upload(vd)) || (rc = d_q.upload(q))) return rc;
    }
    if ((rc = d_out.alloc((size_t)n * (any ? sizeof(int) : sizeof(float4))))) return rc;
    unsigned hc[4] = {n, 0, 0, 0};
    HIPOK(hipMemcpy(h->d_qctr, hc, sizeof(hc), hipMemcpyHostToDevice));
    if ((rc = ensure_ovf(h, h->slot[0]))) return rc;
    if (h->slot[0].stream) HIPOK(hipStreamSynchronize(h->slot[0].stream));
    TraceIO io{};
    io.fetch = h->d_qctr + 1;
    io.ovf = h->slot[0].d_ovf;
    io.stats = h->d_stats;
    io.cull = h->cull;
    io.wide = h->wide;
    if (any) {
        io.squeue = d_q.p;
        io.sray_o = d_o.p;
        io.sray_d = d_d.p;
        io.scount = h->d_qctr;
        io.visible = (int*)d_out.p;
    } else {
        io.queue = d_q.p;
        io.ray_o = d_o.p;
        io.ray_d = d_d.p;
        io.count = h->d_qctr;
        io.hits = (float4*)d_out.p;
    }
    if ((rc = launch_trace(h, io, h->stream))) return rc;
    HIPOK(hipStreamSynchronize(h->stream));
    if (any) HIPOK(hipMemcpy(vis, d_out.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    else HIPOK(hipMemcpy(hits, d_out.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    return RTG_OK;
}

extern "C" {

int rtg_trace_closest(rtg_handle* h, const float* rays, uint32_t n, float* hits) {
    return trace_query(h, rays, n, hits, nullptr, false);
}
int rtg_trace_visible(rtg_handle* h, const float* rays, uint32_t n, int32_t* visible) {
    return trace_query(h, rays, n, nullptr, visible, true);
}

int rtg_debug_capture(rtg_handle* h, int launch) {
    if (!h) return RTG_ERR_ARG;
    if (!RTG_DEBUG) { g_err = "rtg_debug_capture: diagnostic builds only (RTG_DEBUG=1)"; return RTG_ERR_ARG; }
    h->capture_launch = launch;
    return RTG_OK;
}

int rtg_debug_replay(rtg_handle* h, double* out) {
    if (!h || !out) return RTG_ERR_ARG;
#if RTG_DEBUG
    if (!h->d_cap) { g_err = "rtg_debug_replay: nothing captured"; return RTG_ERR_ARG; }
    HIPOK(hipSetDevice(h->device));
    if (int rc = join_frames(h)) return rc;
    HIPOK(hipStreamSynchronize(h->stream));
    unsigned tab[35];
    HIPOK(hipMemcpy(tab, h->d_cap_rays, sizeof(tab), hipMemcpyDeviceToHost));
    const unsigned rays[2] = {tab[33], tab[34]};
    unsigned* d_f8 = nullptr;
    unsigned long long* d_tot = nullptr;
    float* d_out = nullptr;
    HIPOK(hipMalloc((void**)&d_f8, 8 * 32 * sizeof(unsigned)));
    HIPOK(hipMalloc((void**)&d_tot, sizeof(unsigned long long)));
    HIPOK(hipMalloc((void**)&d_out, sizeof(float)));
    hipEvent_t e0, e1;
    HIPOK(hipEventCreate(&e0));
    HIPOK(hipEventCreate(&e1));
    float best = 1e30f;
    unsigned long long tot = 0;
    for (int rep = 0; rep < 3; ++rep) {
        HIPOK(hipMemsetAsync(d_f8, 0, 8 * 32 * sizeof(unsigned), h->stream));
        HIPOK(hipMemsetAsync(d_tot, 0, sizeof(unsigned long long), h->stream));
        HIPOK(hipEventRecord(e0, h->stream));
        hipLaunchKernelGGL(k_replay, dim3(std::max(1, h->trace_blocks[0][0] * RTG_TTB / RTG_TB)), dim3(RTG_TB), 0, h->stream, h->sv, (const uint4*)h->d_cap,
                           (const unsigned*)h->d_cap_len, (const unsigned*)h->d_cap_rays, h->cap_n, 0u, d_f8, d_tot,
                           d_out);
        LAUNCH_OK("k_replay");
        HIPOK(hipEventRecord(e1, h->stream));
        HIPOK(hipEventSynchronize(e1));
        float ms = 0;
        HIPOK(hipEventElapsedTime(&ms, e0, e1));
        best = std::min(best, ms);
        HIPOK(hipMemcpy(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost));
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(d_f8);
    (void)hipFree(d_tot);
    (void)hipFree(d_out);
    out[0] = best;
    out[1] = (double)tot;
    out[2] = rays[0];
    out[3] = rays[1];
    return RTG_OK;
#else
    g_err = "rtg_debug_replay: diagnostic builds only (RTG_DEBUG=1)";
    return RTG_ERR_ARG;
#endif
}

}  // extern "C"
