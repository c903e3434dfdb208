// gemm_nuts.hpp -- mcmc::nuts for the dense Gaussian and the logistic-regression target BEYOND d = 512, on the matrix-product route (included by gemm_samplers.hip,
// inside namespace mi::gemm: it shares gemm_step_kernel, gemm_rowterm_kernel, log_kernel_value and class_sum).
//
// Replaces, for C independent chains, mcmc::internal::nuts_impl with nuts_find_initial_step_size and the recursive nuts_build_tree (ref: src/nuts.cpp:30-332,
// include/mcmc/nuts.ipp:30-241; leap_frog_fn src/nuts.cpp:139-154), identity or DIAGONAL precond_mat, with or without settings.vals_bound (the BOX instantiations below), 1 <= max_tree_depth <= 10.  Before, such a call ran
// on literal_kernel<2>: one workgroup per chain, every leaf of every doubling executed.
//
// The sampler is nuts_lds.hpp's machine -- every doubling on the MEMOISED trajectory (nuts_memo.hpp, DESIGN.md 4.4e: leaf i of a doubling is the state
// LF^{n(i)}(prev_draw, mntm_vec), the 2^j leaves visit 1 + j (j + 1) / 2 distinct points, the U-turn test of a level-l node whose first leaf sits at point n1 compares
// the points n1 and n1 + l); chain states INIT / SEARCH / NEED_DRAW / TREE / DONE; per-chain step, direction, draw index and dual-averaging state -- with the
// evaluation turned inside out: there it is a workgroup collective, here it is ONE product for ALL chains (W = P Theta, resp. eta = X Theta, the row terms, X^T r)
// with the state in HBM as [dimension][chain].  A column of the product is one chain's fma chain over k ascending and columns never mix, so a chain's bits do not
// depend on what its neighbours are doing, or on whether they are finished.  Every chain is asynchronous: its own point of its own doubling of its own draw.
//
// A tick = plain launches on the caller's stream, the same every tick (captured once into a LINEAR hipGraph and replayed while launches are short):
//   nuts_prepare_kernel   element-wise over (dimension, chain), by the column's mode word: the first half-kick and the drift from the chain's last point or from the
//                         origin of a doubling, with the chain's signed step (nuts.cpp:139-154, the roundings of nuts_lds.hpp's DIAGM tick and of literal.hpp);
//                         the draw's Philox normals for the chain's own draw index and p = sqrt(m) z (:200-202); the initial values and z_init (:160-168).
//                         It writes the position buffer the product reads.
//   the product(s)        gemm_step_kernel<EP_NUTS = 12, TGT> (gradient_product): the second half-kick with the step read per column, the gradient stored; a column whose chain takes no point
//                         this tick leaves memory untouched.
//   nuts_point_kernel     one thread per (chain, dimension class j of 4), the layout of gemm_pre_kernel (class_lane): U and K of the new point in the engine's order beyond d = 512
//                         (four strided fma chains, (q0 + q2) + (q1 + q3), one block), the U-turn tests this point closes against the (theta, p) records of
//                         earlier points, the record store; then on the chain's scalars (each of the chain's four lanes keeps a private copy and computes the same):
//                         the walk through the leaves the point unblocks (nuts.ipp:212-239: the same merges, the same uniform per merge from the same Philox slot,
//                         the same early exit), the end of a doubling (the proposal :260-279, the whole tree's test :286-289, the next direction), the end of a
//                         draw (dual averaging :294-302, the kept row, n_accept, nuts_depth), the step-size search (nuts.ipp:30-93), the next state -- and the
//                         column's mode word for the next tick.
// Point records hold theta and p only: the gradient of the last point stays in its own vector (only the next kick reads it).  What a record's gradient was needed for
// -- the origin of the doublings after an accepted proposal -- is an evaluation at the new prev_draw instead (state REGRAD, one tick; the start of every draw
// evaluates at prev_draw anyway: the product runs for every column whether or not its chain uses it).
//
// Nothing waits on the device: no cooperative launch, no grid barrier, no spin, no persistent grid.  The HOST polls a device counter of chains not yet DONE every
// NUTS_POLL_TICKS ticks, up to a ceiling computed from the settings (gemm_nuts_tick_ceiling); a chain still in SEARCH past its allowance is flagged for the literal
// replay (which loops as the reference does), and a ceiling reached with chains still running is an error, never a longer loop.
// Non-finite regime: detected through the energies of every point; the chain is flagged (nf_flag), takes no further part and is replayed by literal_kernel<2>.
// n_leap_out reports the REFERENCE's count (one per leaf walked plus the search), n_exec_out the leapfrogs really made.
// settings.vals_bound (BOX; nuts.cpp:93-135,158-162): the chain lives in the transformed space -- the last point TH, prev_draw, the records and the edges hold theta, X
// holds x = inv_transform(theta), which the product reads; the half-kicks take J(theta) g (the second one in the epilogue EP_NUTS_BOX = 13, the RAW gradient stored),
// U = -(log K(x) + log_jacobian(theta)), K, the records and the U-turn tests run on theta and p, and it is x that leaves (the kept rows, chains.theta).  The unbounded
// instantiations keep their code.

namespace nuts {
enum : int { NS_NEED_DRAW = 0, NS_TREE = 1, NS_DONE = 2, NS_INIT = 3, NS_SEARCH = 4, NS_REGRAD = 5 };
// the column's mode word: what nuts_prepare_kernel does for the chain this tick (zero: nothing -- the product's epilogue leaves the column alone)
enum : uint32_t { CM_IDLE = 0, CM_STEP = 1, CM_ORIGIN = 2, CM_REGRAD = 3, CM_DRAW = 4, CM_INIT = 5 };
// per-(chain, class lane) scalars, [slot][4 Cp] doubles.  nuts_lds.hpp's table: [12 levels][4] pending first halves (n', alpha', n_alpha', proposal point; level 0:
// the draw's kinetic energy, n, alpha, n_alpha) | the dual-averaging state | 12 bit masks over points | alpha and U of every point; then the chain's registers
enum : int {
    SC_DA = 48, SC_OKB = 52, SC_ALPHA = 64, SC_U = 112,
    S_STATE = 160, S_DRAW, S_JD, S_LI, S_NPTS, S_USLOT, S_VDIR, S_SFIRST, S_GOOD, S_PB, S_PB0, S_POSI, S_NEGI,
    S_EPS, S_PREVU, S_ESIGNED, S_H0, S_LOGU, S_NLEAP, S_NEXEC, S_NACC, S_SSTEPS,
    SC_N = 184
};
constexpr int NFIX = 11;          // X, pm, G | prev_draw x 2, its gradient | mntm_vec | the four edge vectors
constexpr int MAX_DEPTH = 10;
}  // namespace nuts

struct TickParams {
    DrawParams lk;           // dK, nK, Cp, term: what log_kernel_value reads
    uint32_t d, dK, n_rec;
    uint64_t C, Cp, Ct, c_off, chain0;       // chains of this range, padded; the call's chains, this range's first column in the caller's arrays, the call's chain0
    size_t vec;
    double *X, *pm, *G;      // the last point: position (the product's B operand), momentum, gradient of log K
    double *prev0, *prev1, *gprev, *mntm;
    double *tpos_t, *tpos_p, *tneg_t, *tneg_p;
    double* rec;             // [n_rec][theta, p][dK][Cp]
    const double *m_sqrt, *m_inv;
    double* sc;
    double* ecol;
    uint32_t *colmode, *pbsel, *didx;
    uint32_t* running;       // chains of the range not yet DONE
    unsigned long long* points;      // (tick, chain) slots in which a chain was not idle: the measurement's
    double* theta;           // [d][Ct]
    double* draws;
    uint64_t *n_accept, *n_leap_out, *n_exec_out;
    double* step;
    uint32_t* depth;
    double* adapt;
    uint32_t* nf_flag;       // [Ct + 1]
    uint64_t seed;
    uint32_t n_burnin, n_total, draw0, n_adapt, max_depth, search_allowance;
    double eps_bar0, delta, gamma, t0, kappa;
    double* TH;              // BOX: theta of the last point in the transformed space (X = inv_transform(TH); prev_draw, the records and the edges hold theta).  Behind the
                             // fields of the unbounded tick, which keep their offsets
};

__global__ void nuts_init_kernel(const TickParams prm)
{
    using namespace nuts;
    const size_t S = 4 * (size_t)prm.Cp;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < S; e += (size_t)gridDim.x * blockDim.x) {
        const uint64_t c = e % prm.Cp;
        const bool live = c < prm.C;
        for (int k = 0; k < SC_N; ++k) prm.sc[(size_t)k * S + e] = 0.0;
        prm.sc[(size_t)S_STATE * S + e] = live ? (double)NS_INIT : (double)NS_DONE;
        prm.sc[(size_t)S_EPS * S + e] = 1.0;
        if (e < prm.Cp) { prm.colmode[c] = live ? (uint32_t)CM_INIT : (uint32_t)CM_IDLE; prm.ecol[c] = 0.0; prm.pbsel[c] = 0u; prm.didx[c] = 0u; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { *prm.running = (uint32_t)prm.C; *prm.points = 0ull; }
}

// one Philox slot -- two dimensions (slot_dims) -- per thread.  BOX (settings.vals_bound): the chain moves in the transformed space -- the half-kick takes J(theta) g
// (nuts.cpp:108-135), the drift moves theta, and x = inv_transform(theta') is what the product reads (:115); the initial values go through transform (:158-162)
template <bool BOX>
__global__ __launch_bounds__(256) void nuts_prepare_kernel(const TickParams prm)
{
    using namespace nuts;
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= prm.Cp) return;
    const uint32_t mode = prm.colmode[c];
    if (mode == CM_IDLE) return;
    const uint32_t slot = blockIdx.y;
    uint32_t dim[2];
    slot_dims(slot, dim[0], dim[1]);
    const double ec = prm.ecol[c];
    const double* prev = prm.pbsel[c] ? prm.prev1 : prm.prev0;
    double z[2] = {0.0, 0.0};
    if (mode == CM_DRAW || mode == CM_INIT)
        slot_normal_pair(prm.seed, prm.chain0 + prm.c_off + c, mode == CM_DRAW ? prm.didx[c] + prm.draw0 : 0u, slot, mode == CM_DRAW ? STREAM_NORMAL : STREAM_INIT, true, prm.d, z[0], z[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t i = dim[h];
        const size_t e = (size_t)i * prm.Cp + c;
        if constexpr (BOX) {
            const BoxParams& bx = prm.lk.bx;
            const bool boxed = bx.blocks[i >> 4] != 0u;      // (both dimensions of a slot sit in one 16-dimension block)
            const int bt = boxed ? bx.bt[i] : 1;
            const double lo = boxed ? bx.lb[i] : 0.0, hi = boxed ? bx.ub[i] : 0.0;
            auto inv = [&](double t) -> double { return boxed ? box_inv_transform(t, bt, lo, hi) : t; };
            if (mode == CM_STEP || mode == CM_ORIGIN) {      // the first half-kick with J(theta) g and the drift of theta, from the last point or from the origin of a doubling
                const bool org = mode == CM_ORIGIN;
                const double th = org ? prev[e] : prm.TH[e], g = org ? prm.gprev[e] : prm.G[e];
                const double jg = boxed ? dfma(box_inv_jacobian(th, bt, lo, hi), g, 0.0) : g;
                const double p = (org ? prm.mntm[e] : prm.pm[e]) + (ec * jg) / 2.0;
                const double tn = th + ec * (prm.m_inv[i] * p);
                prm.pm[e] = p;
                prm.TH[e] = tn;
                prm.X[e] = inv(tn);
            } else if (mode == CM_REGRAD || mode == CM_DRAW) {
                const double p = mode == CM_DRAW ? prm.m_sqrt[i] * z[h] : prm.mntm[e];
                const double th = prev[e];
                if (mode == CM_DRAW) prm.mntm[e] = p;
                prm.pm[e] = p;
                prm.TH[e] = th;
                prm.X[e] = inv(th);
            } else {                                         // CM_INIT: first_draw = transform(initial_vals) (:158-162) and z_init
                const bool in = i < prm.d && c < prm.C;
                const double t = in ? box_transform(prm.theta[(size_t)i * prm.Ct + prm.c_off + c], bx.bt[i], bx.lb[i], bx.ub[i]) : 0.0;
                prm.TH[e] = t;
                prm.prev0[e] = t;
                prm.X[e] = in ? box_inv_transform(t, bx.bt[i], bx.lb[i], bx.ub[i]) : 0.0;
                prm.pm[e] = prm.m_sqrt[i] * z[h];
            }
            continue;
        }
        if (mode == CM_STEP) {                               // the next point from the last one (nuts.cpp:139-154): p += (e g) / 2, theta += e (Minv p)
            const double p = prm.pm[e] + (ec * prm.G[e]) / 2.0;
            prm.pm[e] = p;
            prm.X[e] = prm.X[e] + ec * (prm.m_inv[i] * p);
        } else if (mode == CM_ORIGIN) {                      // ... from the origin of a doubling (prev_draw, mntm_vec: src/nuts.cpp:241-256)
            const double p = prm.mntm[e] + (ec * prm.gprev[e]) / 2.0;
            prm.pm[e] = p;
            prm.X[e] = prev[e] + ec * (prm.m_inv[i] * p);
        } else if (mode == CM_REGRAD) {                      // the gradient at a prev_draw that moved inside the draw
            prm.pm[e] = prm.mntm[e];
            prm.X[e] = prev[e];
        } else if (mode == CM_DRAW) {                        // mntm_vec = sqrt_precond_matrix z (:200-202); the evaluation is at prev_draw
            const double p = prm.m_sqrt[i] * z[h];
            prm.mntm[e] = p;
            prm.pm[e] = p;
            prm.X[e] = prev[e];
        } else {                                             // CM_INIT: first_draw and z_init (:160-168)
            const double x = (i < prm.d && c < prm.C) ? prm.theta[(size_t)i * prm.Ct + prm.c_off + c] : 0.0;
            prm.X[e] = x;
            prm.prev0[e] = x;
            prm.pm[e] = prm.m_sqrt[i] * z[h];
        }
    }
}

template <int TGT, bool BOX>
__global__ __launch_bounds__(256) void nuts_point_kernel(const TickParams prm)
{
    using namespace nuts;
    using mi::lds_nuts::npt_of_dev;
    const ClassLane cl = class_lane();
    const int lane = cl.lane, j = cl.j;
    const uint64_t c = cl.c;
    const uint64_t Cp = prm.Cp;
    const size_t S = 4 * (size_t)Cp;
    double* const sc = prm.sc + ((size_t)j * Cp + c);
    auto SC = [&](int k) -> double& { return sc[(size_t)k * S]; };
    auto any = [&](bool p) -> bool { return __ballot(p) != 0ull; };
    int state = (int)SC(S_STATE);
    if (!any(state != NS_DONE)) return;                  // (wave-uniform: everything below that crosses lanes is executed by the whole wave)
    auto lvl = [&](int l, int f) -> double& { return SC(l * 4 + f); };
    auto okb = [&](int r) -> unsigned long long& { return reinterpret_cast<unsigned long long*>(sc)[(size_t)(SC_OKB + r) * S]; };
    auto pt_alpha = [&](uint32_t n) -> double& { return SC(SC_ALPHA + (int)n); };
    auto pt_U = [&](uint32_t n) -> double& { return SC(SC_U + (int)n); };
    auto prev_K_ = [&]() -> double& { return lvl(0, 0); };
    auto n_val_ = [&]() -> double& { return lvl(0, 1); };
    auto alpha_ = [&]() -> double& { return lvl(0, 2); };
    auto n_alpha_ = [&]() -> double& { return lvl(0, 3); };

    const uint64_t cg = prm.c_off + c;                   // the chain's column in the caller's arrays
    const uint64_t chain = prm.chain0 + cg;
    const uint32_t dK = prm.dK;
    const size_t vec = prm.vec;
    uint32_t draw = (uint32_t)SC(S_DRAW), jd = (uint32_t)SC(S_JD), li = (uint32_t)SC(S_LI), npts = (uint32_t)SC(S_NPTS), uslot = (uint32_t)SC(S_USLOT);
    int vdir = (int)SC(S_VDIR), good_round = (int)SC(S_GOOD), pb = (int)SC(S_PB), pb0 = (int)SC(S_PB0);
    bool s_first = SC(S_SFIRST) != 0.0, pos_init = SC(S_POSI) != 0.0, neg_init = SC(S_NEGI) != 0.0;
    double eps = SC(S_EPS), prev_U = SC(S_PREVU), e_signed = SC(S_ESIGNED), H0 = SC(S_H0), log_u = SC(S_LOGU);
    double n_leap = SC(S_NLEAP), n_exec = SC(S_NEXEC), n_acc = SC(S_NACC), s_steps = SC(S_SSTEPS);
    bool nf = false;
    const double log_half = det_log(0.5), neg_log2 = -det_log(2.0);
    const bool run = state == NS_TREE, init = state == NS_INIT, srch = state == NS_SEARCH, nd = state == NS_NEED_DRAW, rg = state == NS_REGRAD;
    const unsigned long long busy = __ballot(state != NS_DONE) & 0xffffull;      // (lanes 0 .. 15: one per chain of the wave)
    if (lane == 0) atomicAdd(prm.points, (unsigned long long)__builtin_popcountll(busy));
    auto pvec = [&](int b) -> double* { return b ? prm.prev1 : prm.prev0; };
    const double* const pos = BOX ? prm.TH : prm.X;      // the point as the chain sees it: with bounds theta, in the transformed space (K, the records, the U-turn tests)

    // ------------------------------------------------------------ the new point: K, U, its record, the far edge of the tree, the gradient at prev_draw
    const uint32_t mpt = npts + 1u;                      // the point this tick computed (run lanes)
    const bool rec_ok = mpt <= prm.n_rec;                // (always: a doubling of depth jd < max_tree_depth has 1 + jd (jd + 1) / 2 points)
    if (run && !rec_ok) nf = true;
    uint32_t pmask = (run && rec_ok) ? (uint32_t)mi::lds_nuts::pm_table.v[jd < 10u ? jd : 9u][mpt < 48u ? mpt : 0u] : 0u;
    double pK;
    {
        double* const rt = prm.rec + (size_t)((run && rec_ok) ? mpt - 1u : 0u) * 2 * vec;
        double* const rp = rt + vec;
        const bool st_rec = run && rec_ok;
        const bool st_edge = st_rec && (mpt == 1u + jd);     // the first leaf of the second half: what a successful doubling leaves in draw_pos / draw_neg
        double* const et = (vdir > 0) ? prm.tpos_t : prm.tneg_t;
        double* const ep = (vdir > 0) ? prm.tpos_p : prm.tneg_p;
        const bool keepg = nd || rg || init;
        double qk = 0.0;
#pragma unroll 4
        for (uint32_t i = (uint32_t)j; i < dK; i += 4u) {
            const size_t e = (size_t)i * Cp + c;
            const double x = pos[e], p = prm.pm[e];
            qk = dfma(p, prm.m_inv[i] * p, qk);              // K = p . (Minv p) / 2 (nuts.ipp:51,66,140; nuts.cpp:204)
            if (st_rec) { rt[e] = x; rp[e] = p; }
            if (st_edge) { et[e] = x; ep[e] = p; }
            if (keepg) prm.gprev[e] = prm.G[e];
        }
        if (st_edge) { if (vdir > 0) pos_init = false; else neg_init = false; }
        pK = class_sum(qk) / 2.0;
    }
    double val = log_kernel_value<TGT>(prm.lk, prm.X, prm.G, c, j);
    if constexpr (BOX) val = val + box_log_jacobian(prm.lk, prm.TH, c, lane);      // box_log_kernel (nuts.cpp:93-104): log K(x) + log_jacobian(theta)
    // ------------------------------------------------------------ the U-turn tests this point closes: level l against point mpt - l (nuts.ipp:224-229)
    while (any(pmask != 0u)) {
        const bool t = pmask != 0u;
        const uint32_t l = t ? (uint32_t)__builtin_ctz(pmask) : 1u;
        const double* const rt = prm.rec + (size_t)(t ? mpt - l - 1u : 0u) * 2 * vec;
        const double* const rp = rt + vec;
        double r1 = 0.0, r2 = 0.0;
#pragma unroll 4
        for (uint32_t i = (uint32_t)j; i < dK; i += 4u) {
            const size_t e = (size_t)i * Cp + c;
            const double tb = t ? rt[e] : 0.0, pbv = t ? rp[e] : 0.0;
            const double x = pos[e], p = prm.pm[e];
            const double dd = (vdir > 0) ? (x - tb) : (tb - x);
            r1 = dfma(dd, pbv, r1);
            r2 = dfma(dd, p, r2);
        }
        r1 = class_sum(r1); r2 = class_sum(r2);
        if (t) {
            const unsigned long long bit = 1ull << (mpt - l);
            const bool ok = (r1 >= 0.0) && (r2 >= 0.0);
            okb((int)l) = (okb((int)l) & ~bit) | (ok ? bit : 0ull);
            pmask &= pmask - 1u;
        }
    }

    // SEARCH ends (or is skipped by a continuation): the dual-averaging state of nuts.cpp:174-176
    auto start_sampling = [&](bool p) {
        if (p) {
            SC(SC_DA + 2) = det_log(10 * eps);               // nuts.cpp:174
            SC(SC_DA) = 0.0;
            const uint32_t g0 = prm.draw0 + draw;
            SC(SC_DA + 1) = (g0 == 0u) ? prm.eps_bar0 : eps;
            if (g0 > 0u && g0 <= prm.n_adapt && prm.adapt != nullptr) {      // a continuation inside the adaptation window
                SC(SC_DA) = prm.adapt[cg]; SC(SC_DA + 1) = prm.adapt[prm.Ct + cg]; SC(SC_DA + 2) = prm.adapt[2 * prm.Ct + cg];
            }
            state = NS_NEED_DRAW;
        }
    };
    auto begin_doubling = [&](bool p) {                      // direction draw, nuts.cpp:233-235
        if (p) {
            const double zdir = rng_uniform(prm.seed, chain, draw + prm.draw0, uslot);
            uslot++;
            vdir = (zdir <= 0.5) ? -1 : 1;
            e_signed = (double)vdir * eps;
            H0 = prev_U + prev_K_();
            li = 0; npts = 0;
        }
    };

    double pU = -val;                                    // nuts.ipp:134-138 / :50,65
    const bool u_nf = !is_finite(pU);
    // ---- INIT: the chain's first state is on record (prev_draw by nuts_prepare_kernel, its gradient above); SEARCH: one step of nuts_find_initial_step_size
    if (init) {
        prev_U = pU;                                     // nuts.cpp:181 (no finiteness guard there)
        if (u_nf || !is_finite(pK)) nf = true;
        H0 = (u_nf ? INF : pU) + pK;                     // U0 + K0 (nuts.ipp:50-52)
        s_first = true; s_steps = 0.0;
        pb = 0; pb0 = 0;
        if (prm.draw0 != 0u) {                           // a continuation call: the step size comes back in
            eps = prm.step ? prm.step[cg] : 1.0;
            start_sampling(true);
        } else state = NS_SEARCH;
    }
    if (srch) {
        if (u_nf || !is_finite(pK)) nf = true;
        const double dH = -((u_nf ? INF : pU) + pK) + H0;                // nuts.ipp:68,86
        vdir = 2 * (dH > log_half ? 1 : 0) - 1;                          // :75,88
        s_first = false;
        start_sampling(!(dH > neg_log2));                                // :78,90: the loop ends
    }
    // ---- the start of a draw (:200-219): the momentum is in place, K above; the gradient at prev_draw was kept above
    if (nd) {
        prev_K_() = pK;                                  // :204
        log_u = det_log(rng_uniform(prm.seed, chain, draw + prm.draw0, 0u)) - prev_U - pK;      // :206
        pb0 = pb; pos_init = true; neg_init = true;
        uslot = 1;
        jd = 0; n_val_() = 1.0; alpha_() = 0.0; n_alpha_() = 0.0; good_round = 0;
        state = NS_TREE;
        begin_doubling(true);
    }
    if (rg) state = NS_TREE;                             // (its doubling has begun: begin_doubling ran when the last one ended)
    if (u_nf) { pU = INF; if (run) nf = true; }
    if (run && !is_finite(pK)) nf = true;
    // ---- the point's scalars (nuts.ipp:146-157): n', s' as bits, alpha and U in the chain's table
    if (run && rec_ok) {
        const double dH_pt = -(pU + pK) + H0;
        const double ca_pt = det_exp((dH_pt < 0.0) ? dH_pt : 0.0);       // :157
        const unsigned long long bit = 1ull << mpt;
        const bool cn_b = log_u <= -pU - pK;             // :146
        const bool cs_b = log_u < 1000.0 - pU - pK;      // :147
        okb(0) = (okb(0) & ~bit) | (cn_b ? bit : 0ull);
        okb(11) = (okb(11) & ~bit) | (cs_b ? bit : 0ull);
        pt_alpha(mpt) = ca_pt; pt_U(mpt) = pU;
        n_exec += 1.0;
        npts = mpt;
    }
    // ------------------------------------------------------------ walk the leaves this point unblocks (nuts.ipp:146-158, 212-239): leaf after leaf as the recursion
    // returns through them, on the memoised scalars (nuts_lds.hpp, section C)
    bool wl = run && rec_ok;                             // (the leaf a chain waits at sits on its newest point)
    bool at_fin = false, complete = false;
    double cn = 0.0, cna = 0.0, ca = 0.0;
    uint32_t cref = 0;
    uint32_t n = npt_of_dev(li);
#pragma unroll 1
    while (wl) {
        const uint32_t t1 = (uint32_t)__builtin_ctz(~li);
        const uint32_t nn = n + (t1 + 1u) - t1 * (t1 + 1u) / 2u;         // the point of leaf li + 1
        const unsigned long long nbit = 1ull << n;
        cn = (okb(0) & nbit) ? 1.0 : 0.0;
        ca = pt_alpha(n);
        cna = 1.0; cref = n;
        bool failed = !(okb(11) & nbit);
        n_leap += 1.0;
        uint32_t pend_level = jd + 1;
#pragma unroll 1
        for (uint32_t l = 1; l <= (uint32_t)MAX_DEPTH; ++l) {
            if (l > jd) break;                                           // reached the root of its own tree
            const bool bit = ((li >> (l - 1)) & 1u) != 0u;
            if (!failed && !bit) { pend_level = l; break; }              // first half: wait here
            if (!bit) continue;
            const double z = rng_uniform(prm.seed, chain, draw + prm.draw0, uslot);  // :213
            uslot++;
            const double p_n = lvl((int)l, 0), p_a = lvl((int)l, 1), p_na = lvl((int)l, 2);
            const double prob = cn / (p_n + cn);                         // :212
            if (!(z < prob)) cref = (uint32_t)lvl((int)l, 3);            // keep new_draw_p (:215-217): a point of the trajectory, by reference
            cn = p_n + cn;                                               // :220-222
            ca = p_a + ca;
            cna = p_na + cna;
            if (!failed) {                                               // :226-229, evaluated when its second point appeared
                const uint32_t n1 = n - l * (l + 1u) / 2u;               // the node's first leaf: li with its l low (set) bits cleared
                if (!((okb((int)l) >> n1) & 1ull)) failed = true;
            }
        }
        const bool keep = !failed;
        complete = keep && (li == (1u << jd) - 1u);
        if (keep && !complete) {                         // a pending first half: its scalars, the proposal by reference
            lvl((int)pend_level, 0) = cn; lvl((int)pend_level, 1) = ca;
            lvl((int)pend_level, 2) = cna; lvl((int)pend_level, 3) = (double)cref;
            li = li + 1u; n = nn;
            wl = nn <= npts;
        } else {
            at_fin = true; wl = false;
        }
    }
    // ------------------------------------------------------------ end of a doubling: top-level accept first (src/nuts.cpp:260-279).  The proposal is a point of the
    // trajectory: its record becomes prev_draw
    bool take = false;
    if (complete) {
        const double z = rng_uniform(prm.seed, chain, draw + prm.draw0, uslot);      // :261
        uslot++;
        take = z < cn / n_val_();                        // :263
        if (take) { prev_U = pt_U(cref); good_round = 1; pb = 1 - pb0; }             // :264-277
    }
    if (any(take)) {
        const double* const src = prm.rec + (size_t)(take ? cref - 1u : 0u) * 2 * vec;
        double* const dst = pvec(1 - pb0);
        if (take)
#pragma unroll 4
            for (uint32_t i = (uint32_t)j; i < dK; i += 4u) { const size_t e = (size_t)i * Cp + c; dst[e] = src[e]; }
    }
    // ---- the whole tree's U-turn test (:286-289)
    bool s_ok = false;
    if (any(complete)) {
        const double* const en_t = neg_init ? pvec(pb0) : prm.tneg_t;
        const double* const en_p = neg_init ? prm.mntm : prm.tneg_p;
        const double* const ep_t = pos_init ? pvec(pb0) : prm.tpos_t;
        const double* const ep_p = pos_init ? prm.mntm : prm.tpos_p;
        double r1 = 0.0, r2 = 0.0;
#pragma unroll 4
        for (uint32_t i = (uint32_t)j; i < dK; i += 4u) {
            const size_t e = (size_t)i * Cp + c;
            const double dd = complete ? ep_t[e] - en_t[e] : 0.0;
            r1 = dfma(dd, complete ? en_p[e] : 0.0, r1);
            r2 = dfma(dd, complete ? ep_p[e] : 0.0, r2);
        }
        r1 = class_sum(r1); r2 = class_sum(r2);
        s_ok = complete && (r1 >= 0.0) && (r2 >= 0.0);
    }
    bool row = false;
    uint32_t row_idx = 0;
    if (at_fin) {
        alpha_() = ca; n_alpha_() = cna; n_val_() = n_val_() + cn;       // :246,255 ; :283
        const bool more = s_ok && (jd + 1 < prm.max_depth);
        jd = jd + 1;                                                     // :284
        if (!more) {                                                     // the end of the draw: dual averaging nuts.cpp:294-302
            if (prm.depth && j == 0) prm.depth[(size_t)draw * prm.Ct + cg] = jd;
            if (draw + prm.draw0 < prm.n_adapt) {
                const double it = (double)(draw + prm.draw0 + 1);
                const double h_new = SC(SC_DA) + (1.0 / (it + prm.t0)) * (prm.delta - (alpha_() / n_alpha_()) - SC(SC_DA));
                SC(SC_DA) = h_new;
                eps = det_exp(SC(SC_DA + 2) - h_new * __builtin_sqrt(it) / prm.gamma);
                const double eb = SC(SC_DA + 1);
                SC(SC_DA + 1) = eb * det_exp(det_pow(it, -prm.kappa) * (det_log(eps) - det_log(eb)));
            } else eps = SC(SC_DA + 1);
            if (draw >= prm.n_burnin) { n_acc += (double)good_round; row = prm.draws != nullptr; row_idx = draw - prm.n_burnin; }
            draw++;
            state = NS_NEED_DRAW;
        } else {
            begin_doubling(true);
            if (take) state = NS_REGRAD;                 // prev_draw moved: the next doubling's origin needs its gradient
        }
    }
    // a chain leaves: flagged (replayed from its initial state: nothing of it is kept), or with its last draw made
    const bool flagged = nf && state != NS_DONE;
    const bool retire = !flagged && state == NS_NEED_DRAW && draw >= prm.n_total;
    if (any(row || retire)) {
        const double* const src = pvec(pb);
        double* const out = row ? prm.draws + (size_t)row_idx * prm.d * prm.Ct + cg : nullptr;
        constexpr int UNROLL = BOX ? 1 : 4;              // (the bounded loop calls out of line)
        if (row || retire)
#pragma unroll UNROLL
            for (uint32_t i = (uint32_t)j; i < prm.d; i += 4u) {
                double v = src[(size_t)i * Cp + c];
                if constexpr (BOX) {                         // it is x = inv_transform(theta) that leaves (nuts.cpp: the final inv_transform of draws_out)
                    const BoxParams& bx = prm.lk.bx;
                    if (bx.blocks[i >> 4] != 0u) v = box_inv_transform(v, bx.bt[i], bx.lb[i], bx.ub[i]);
                }
                if (row && !flagged) out[(size_t)i * prm.Ct] = v;                   // nuts.cpp:306-309
                if (retire) prm.theta[(size_t)i * prm.Ct + cg] = v;
            }
    }
    if (flagged || retire) {
        if (j == 0) {
            if (flagged) { if (prm.nf_flag) { prm.nf_flag[cg] = 1u; prm.nf_flag[prm.Ct] = 1u; } }
            else {                                       // final counters, step size and dual-averaging state (nuts.cpp:311-330)
                if (prm.n_accept) prm.n_accept[cg] = (uint64_t)n_acc;
                if (prm.n_leap_out) prm.n_leap_out[cg] = (uint64_t)n_leap;
                if (prm.n_exec_out) prm.n_exec_out[cg] = (uint64_t)n_exec;
                if (prm.step) prm.step[cg] = eps;
                if (prm.adapt) { prm.adapt[cg] = SC(SC_DA); prm.adapt[prm.Ct + cg] = SC(SC_DA + 1); prm.adapt[2 * prm.Ct + cg] = SC(SC_DA + 2); }
            }
            atomicSub(prm.running, 1u);
        }
        state = NS_DONE;
    }
    // ------------------------------------------------------------ what the chain does next tick
    uint32_t mode = CM_IDLE;
    double ec = 0.0;
    if (state == NS_SEARCH) {                            // the step of the next leapfrog (nuts.ipp:62, 80-82)
        if (s_steps >= (double)prm.search_allowance) {   // past its allowance: the literal replay loops as the reference does
            if (j == 0) { if (prm.nf_flag) { prm.nf_flag[cg] = 1u; prm.nf_flag[prm.Ct] = 1u; } atomicSub(prm.running, 1u); }
            state = NS_DONE;
        } else {
            if (!s_first) eps = eps * ((vdir == 1) ? 2.0 : 0.5);
            n_leap += 1.0; n_exec += 1.0; s_steps += 1.0;
            mode = CM_STEP; ec = eps;
        }
    } else if (state == NS_TREE) { mode = (npts == 0u) ? (uint32_t)CM_ORIGIN : (uint32_t)CM_STEP; ec = e_signed; }
    else if (state == NS_REGRAD) mode = CM_REGRAD;
    else if (state == NS_NEED_DRAW) mode = CM_DRAW;
    if (j == 0) { prm.colmode[c] = mode; prm.ecol[c] = ec; prm.pbsel[c] = (uint32_t)pb; prm.didx[c] = draw; }
    SC(S_STATE) = (double)state; SC(S_DRAW) = (double)draw; SC(S_JD) = (double)jd; SC(S_LI) = (double)li; SC(S_NPTS) = (double)npts; SC(S_USLOT) = (double)uslot;
    SC(S_VDIR) = (double)vdir; SC(S_SFIRST) = s_first ? 1.0 : 0.0; SC(S_GOOD) = (double)good_round; SC(S_PB) = (double)pb; SC(S_PB0) = (double)pb0;
    SC(S_POSI) = pos_init ? 1.0 : 0.0; SC(S_NEGI) = neg_init ? 1.0 : 0.0;
    SC(S_EPS) = eps; SC(S_PREVU) = prev_U; SC(S_ESIGNED) = e_signed; SC(S_H0) = H0; SC(S_LOGU) = log_u;
    SC(S_NLEAP) = n_leap; SC(S_NEXEC) = n_exec; SC(S_NACC) = n_acc; SC(S_SSTEPS) = s_steps;
}

// ---- host side
constexpr uint32_t NUTS_POLL_TICKS = 32;             // the counter of running chains comes back every so many ticks
constexpr uint32_t NUTS_SEARCH_TICKS = 4096;         // the allowance of nuts_find_initial_step_size (it doubles or halves the step: 2^+-1100 is the end of fp64)

uint32_t gemm_nuts_points(uint32_t max_depth) { return 1u + (max_depth - 1u) * max_depth / 2u; }      // of the deepest doubling (depth max_depth - 1)
// ticks a chain needs at most: INIT, the search's allowance (a fresh run), and per draw the evaluation at prev_draw, one REGRAD per doubling that is not the
// last, and every point of every doubling: sum over j < max_depth of (1 + j (j + 1) / 2)
uint64_t gemm_nuts_tick_ceiling(uint32_t max_depth, uint64_t n_total, bool search)
{
    uint64_t pts = 0;
    for (uint64_t j = 0; j < max_depth; ++j) pts += 1 + j * (j + 1) / 2;
    return 1 + (search ? (uint64_t)NUTS_SEARCH_TICKS + 1 : 0) + n_total * (1 + (uint64_t)(max_depth - 1) + pts);
}
// The workspace of a range of Cp columns (gemm_samplers.hip: Carve): first what does not depend on the chains -- the packed matrices, the counters --, then per chain the
// fixed vectors and 2 (theta, p) x gemm_nuts_points record vectors of gemm_padded_d(d) doubles, the logistic target's two row-term vectors, the scalars, the column words;
// with bounds ONE more vector behind them all: theta of the last point (the eleven fixed vectors keep their places)
struct NutsWs : TargetWs {
    double* ctr;               // 32 doubles: the two counters
    double* fix[nuts::NFIX];   // X, pm, G | prev_draw x 2, its gradient | mntm_vec | the four edge vectors
    double* rec;
    double *sc, *ecol;
    uint32_t *colmode, *pbsel, *didx;
    double* th;                // vals_bound: theta of the last point
    size_t fixed, n_doubles;   // doubles that do not depend on the chains, and all of them
};
static NutsWs gemm_nuts_carve(uint32_t d, uint32_t n_rows, uint32_t max_depth, uint64_t Cp, bool bounded, double* base)
{
    NutsWs w{};
    w.l = layout_of(d, n_rows, Cp);
    const Layout& l = w.l;
    Carve cv{base};
    take_matrices(cv, w);
    w.ctr = cv.take(32);
    w.fixed = cv.n;
    for (double*& v : w.fix) v = cv.take(l.vec);
    w.rec = cv.take(2 * (size_t)gemm_nuts_points(max_depth) * l.vec);
    take_row_terms(cv, w);
    w.sc = cv.take(4 * (size_t)nuts::SC_N * l.Cp);
    w.ecol = cv.take(l.Cp);
    w.colmode = reinterpret_cast<uint32_t*>(cv.take(2 * l.Cp));              // 3 Cp words in 2 Cp doubles
    w.pbsel = w.colmode + l.Cp; w.didx = w.pbsel + l.Cp;
    if (bounded) w.th = cv.take(l.vec);
    w.n_doubles = cv.n;
    return w;
}
// bytes per chain (every region behind the fixed ones is a multiple of the columns: one column counts them), and of what does not depend on the chains
size_t gemm_nuts_chain_bytes(uint32_t d, uint32_t n_rows, uint32_t max_depth, bool bounded)
{
    const NutsWs w = gemm_nuts_carve(d, n_rows, max_depth, 1, bounded, nullptr);
    return (w.n_doubles - w.fixed) * sizeof(double);
}
size_t gemm_nuts_fixed_bytes(uint32_t d, uint32_t n_rows) { return gemm_nuts_carve(d, n_rows, 1, 1, false, nullptr).fixed * sizeof(double); }
// chains per range when `budget` bytes are there for the route's own workspace: all of them (rounded up to the chain tile) if they fit, else the largest multiple
// of 128 that does; 0: not even one tile -- the call stays on the literal kernel
uint64_t gemm_nuts_range_chains(uint64_t C, size_t chain_bytes, size_t fixed_bytes, size_t budget)
{
    const uint64_t Cp = padded_chains(C);
    if (budget < fixed_bytes || chain_bytes == 0) return 0;
    const uint64_t fit = (budget - fixed_bytes) / chain_bytes / TN * TN;
    return fit < Cp ? fit : Cp;
}

template <int TGT, bool BOX>
static int gemm_nuts_run_t(GemmNutsRun& r, hipStream_t st, const char** kernel_name)
{
    if (r.max_depth < 1 || r.max_depth > (uint32_t)nuts::MAX_DEPTH || r.C == 0) return (int)hipErrorInvalidValue;      // (the caller routes these elsewhere)
    if (BOX && (!r.btype || !r.lb || !r.ub || !r.box_blocks)) return (int)hipErrorInvalidValue;
    const uint32_t n_rows = TGT == TGT_LOGISTIC ? r.n_rows : 0u;
    const NutsWs w = gemm_nuts_carve(r.d, n_rows, r.max_depth, padded_chains(r.C), BOX, static_cast<double*>(r.ws));
    const Layout& l = w.l;
    TickParams tp{};
    tp.d = r.d; tp.dK = l.dK; tp.n_rec = gemm_nuts_points(r.max_depth); tp.C = r.C; tp.Cp = l.Cp; tp.Ct = r.C_total; tp.c_off = r.c_off; tp.chain0 = r.chain0; tp.vec = l.vec;
    tp.X = w.fix[0]; tp.pm = w.fix[1]; tp.G = w.fix[2]; tp.prev0 = w.fix[3]; tp.prev1 = w.fix[4]; tp.gprev = w.fix[5]; tp.mntm = w.fix[6];
    tp.tpos_t = w.fix[7]; tp.tpos_p = w.fix[8]; tp.tneg_t = w.fix[9]; tp.tneg_p = w.fix[10];
    tp.TH = w.th;
    if (BOX) { tp.lk.bx.bt = r.btype; tp.lk.bx.lb = r.lb; tp.lk.bx.ub = r.ub; tp.lk.bx.blocks = r.box_blocks; }
    tp.rec = w.rec; tp.sc = w.sc; tp.ecol = w.ecol; tp.colmode = w.colmode; tp.pbsel = w.pbsel; tp.didx = w.didx;
    tp.running = reinterpret_cast<uint32_t*>(w.ctr);
    tp.points = reinterpret_cast<unsigned long long*>(w.ctr + 1);
    tp.lk.dK = l.dK; tp.lk.nK = l.nK; tp.lk.Cp = l.Cp; tp.lk.C = r.C; tp.lk.d = r.d; tp.lk.term = w.term;
    tp.m_sqrt = r.mass_tables + l.dK; tp.m_inv = r.mass_tables + 2 * (size_t)l.dK;
    tp.theta = r.theta; tp.draws = r.draws; tp.n_accept = r.n_accept; tp.n_leap_out = r.n_leap; tp.n_exec_out = r.n_exec; tp.step = r.step; tp.depth = r.depth;
    tp.adapt = r.adapt; tp.nf_flag = r.nf_flag;
    tp.seed = r.seed; tp.n_burnin = r.n_burnin; tp.n_total = r.n_burnin + r.n_keep; tp.draw0 = r.draw0; tp.n_adapt = r.n_adapt; tp.max_depth = r.max_depth;
    tp.search_allowance = NUTS_SEARCH_TICKS;
    tp.eps_bar0 = r.eps_bar0; tp.delta = r.delta; tp.gamma = r.gamma; tp.t0 = r.t0; tp.kappa = r.kappa;

    if (int e = step_attrs<TGT>()) return e;
    if (r.pack) pack_target<TGT>(w, r.P, r.X, r.n_rows, r.d, st);      // (the matrices are the same for every range of a call)
    hipLaunchKernelGGL(nuts_init_kernel, dim3(stride_grid(4 * l.Cp)), dim3(256), 0, st, tp);
    GEMM_TRY(hipGetLastError());

    const uint32_t n_ntiles = (uint32_t)(l.Cp / TN);
    const unsigned cls_grid = (unsigned)(l.Cp / 64);
    const dim3 prep_grid((unsigned)(l.Cp / 256 + (l.Cp % 256 ? 1 : 0)), l.dK / 2);
    // the launches of ONE tick: the same every tick (what differs lives in device memory)
    auto enqueue_tick = [&](hipStream_t s) -> int {
        hipLaunchKernelGGL(nuts_prepare_kernel<BOX>, prep_grid, dim3(256), 0, s, tp);
        StepParams sp{};
        sp.n_ntiles = n_ntiles; sp.Cp = l.Cp; sp.pm = tp.pm; sp.pos = tp.X; sp.g_out = tp.G; sp.ecol = tp.ecol; sp.colmode = tp.colmode;
        if (BOX) { sp.pos = tp.TH; sp.xpos = tp.X; sp.bt = r.btype; sp.lb = r.lb; sp.ub = r.ub; sp.box_blocks = r.box_blocks; }
        if (int e = gradient_product<TGT>(w, r.y, r.n_rows, tp.X, BOX ? EP_NUTS_BOX : EP_NUTS, sp, s)) return e;
        hipLaunchKernelGGL((nuts_point_kernel<TGT, BOX>), dim3(cls_grid), dim3(256), 0, s, tp);
        return (int)hipGetLastError();
    };

    // one tick captured once (a linear graph), replayed; the host polls the counter of running chains every NUTS_POLL_TICKS ticks, up to the ceiling
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    const bool graphed = r.use_graph && capture_and_instantiate(enqueue_tick, &graph, &exec);
    const uint64_t ceiling = gemm_nuts_tick_ceiling(r.max_depth, (uint64_t)r.n_burnin + r.n_keep, r.draw0 == 0);
    uint64_t ticks = 0;
    uint32_t running = (uint32_t)r.C;
    int rc = 0;
    while (rc == 0 && running != 0u && ticks < ceiling) {
        const uint64_t n = std::min<uint64_t>(NUTS_POLL_TICKS, ceiling - ticks);
        for (uint64_t t = 0; t < n && rc == 0; ++t) rc = graphed ? (int)hipGraphLaunch(exec, st) : enqueue_tick(st);
        ticks += n;
        if (rc == 0) rc = (int)hipMemcpyAsync(&running, tp.running, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (rc == 0) rc = (int)hipStreamSynchronize(st);
    }
    unsigned long long points = 0;
    if (rc == 0) rc = (int)hipMemcpy(&points, tp.points, sizeof(points), hipMemcpyDeviceToHost);
    if (graphed) { const int e = release_graph(st, graph, exec); if (rc == 0) rc = e; }
    if (rc) return rc;
    r.ticks_run = ticks; r.points_taken = points; r.still_running = running;
    if (kernel_name) {
        static thread_local char name[112];
        snprintf(name, sizeof(name), "gemm_step_kernel<%d, %d> (nuts, memoised%s%s%s)", (int)(BOX ? EP_NUTS_BOX : EP_NUTS), TGT, graphed ? ", graph" : "",
                 r.diag_mass ? ", diagonal precond_mat" : "", BOX ? ", bounds" : "");
        *kernel_name = name;
    }
    return 0;
}

int gemm_nuts_run(GemmNutsRun& r, hipStream_t st, const char** kernel_name)
{
    if (r.bounded) return r.X != nullptr ? gemm_nuts_run_t<TGT_LOGISTIC, true>(r, st, kernel_name) : gemm_nuts_run_t<TGT_DENSE, true>(r, st, kernel_name);
    return r.X != nullptr ? gemm_nuts_run_t<TGT_LOGISTIC, false>(r, st, kernel_name) : gemm_nuts_run_t<TGT_DENSE, false>(r, st, kernel_name);
}
