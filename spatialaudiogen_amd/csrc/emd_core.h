// Exact EMD-hat between two non-negative histograms on a metric ground distance (pyemd 0.5.1 `emd` with its default extra-mass
// penalty, as the reference calls it: distance.py:100-130, eval.py:188-193):
//
//   EMD-hat(P, Q) = min sum_ij f_ij C_ij   s.t. f >= 0, sum_j f_ij <= P_i, sum_i f_ij <= Q_j, sum_ij f_ij = min(sum P, sum Q)
//                 + |sum P - sum Q| * max C
//
// in fp64, exactly (pyemd rounds masses and costs to 1e6 levels first).  Steps:
//   1. min(P_i, Q_i) stays at node i at zero cost (FastEMD's metric shortcut: valid because C is a metric).  What is left is a
//      transportation problem from the supply nodes (P_i > Q_i) to the demand nodes (Q_j > P_j) - two disjoint sets, so its cost
//      and flow blocks are at most (n/2)^2 entries.
//   2. Successive shortest paths: Dijkstra on reduced costs (node potentials keep them >= 0) from every source with supply left to
//      the nearest sink with demand left, augment by the bottleneck, repeat until the supply or the demand is used up.  The flow
//      value then equals min(sum P, sum Q) - sum_i min(P_i, Q_i), i.e. the excess never moves (a zero-cost slack node).
//   Ties: the smaller (distance, index) pair wins everywhere, so the result is a pure function of the inputs.
//
// The same code runs on the device (one wave per problem, state in LDS, lanes parallel over the sinks / sources; EmdWave in
// evalx.hip) and on the host (EmdSerial below: one "lane" that covers every index), so the algorithm is tested on the CPU
// (tests/test_eval_metrics_host.py) before the device runs it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define EMD_FN __host__ __device__ __forceinline__
#else
#define EMD_FN inline
#endif

namespace sagen {

constexpr int EMD_MAX_NODES = 96;                                  // <= 2 nodes per lane of a wave64
constexpr int EMD_MAX_BLOCK = (EMD_MAX_NODES / 2) * (EMD_MAX_NODES / 2);
constexpr int EMD_MAX_AUGMENT = 4096;                               // augmentations per problem before "not converged"

// solver state (LDS on the device)
struct EmdState {
    double cst[EMD_MAX_BLOCK];       // C[src[i]][snk[j]] at i * nd + j
    double flw[EMD_MAX_BLOCK];       // flow on (i, j)
    double sup[EMD_MAX_NODES], dem[EMD_MAX_NODES];   // supply / demand left
    double ps[EMD_MAX_NODES], pt[EMD_MAX_NODES];     // potentials of sources / sinks
    double ds[EMD_MAX_NODES], dt[EMD_MAX_NODES];     // Dijkstra labels
    int src[EMD_MAX_NODES], snk[EMD_MAX_NODES];
    int pred_t[EMD_MAX_NODES], pred_s[EMD_MAX_NODES];   // sink <- source on the tree; source <- sink (-1: a root)
    int done_t[EMD_MAX_NODES], done_s[EMD_MAX_NODES];
    int list[EMD_MAX_NODES];         // sources reached in the current step
    int ns, nd;
    double dmin;
    int jmin;
};

// the host "wave": one lane that walks every index; the cross-lane steps are the identity
struct EmdSerial {
    static constexpr int WIDTH = 1;
    int lane() const { return 0; }
    void sync() const {}
    void argmin(double& d, int& i) const { (void)d; (void)i; }
    double sum(double v) const { return v; }
    double max(double v) const { return v; }
    int any(bool b) const { return b ? 1 : 0; }
    // position of this lane's flagged entry in a list that grows in index order; `count` = entries so far (uniform)
    int prefix(bool f, int& count) const { const int p = count; count += f ? 1 : 0; return p; }
};

EMD_FN bool emd_less(double d2, int i2, double d, int i) { return d2 < d || (d2 == d && i2 < i); }

// P, Q [n]: masses (finite, >= 0); C [n*n] row-major fp64 metric.  Returns the transport part of EMD-hat (without the penalty);
// *converged = 0 if the augmentation cap was hit or no path was found.
template <class W>
EMD_FN double emd_transport(const W& w, EmdState& st, const double* P, const double* Q, int n, const double* C, int* converged) {
    const int lane = w.lane(), WD = W::WIDTH;
    const double INF = 1e300;
    if (lane == 0) {                                        // 1. the metric shortcut; sources / sinks in node order
        int ns = 0, nd = 0;
        for (int v = 0; v < n; ++v) {
            const double m = P[v] < Q[v] ? P[v] : Q[v];
            const double a = P[v] - m, b = Q[v] - m;
            if (a > 0.0) { st.src[ns] = v; st.sup[ns] = a; ++ns; }
            else if (b > 0.0) { st.snk[nd] = v; st.dem[nd] = b; ++nd; }
        }
        st.ns = ns; st.nd = nd;
    }
    w.sync();
    const int ns = st.ns, nd = st.nd;
    for (int e = lane; e < ns * nd; e += WD) {
        const int i = e / nd, j = e - (e / nd) * nd;
        st.cst[e] = C[(long)st.src[i] * n + st.snk[j]];
        st.flw[e] = 0.0;
    }
    for (int i = lane; i < ns; i += WD) st.ps[i] = 0.0;
    for (int j = lane; j < nd; j += WD) st.pt[j] = 0.0;
    w.sync();
    int ok = 1;
    for (int it = 0;; ++it) {
        int has_s = 0, has_d = 0;
        for (int i = lane; i < ns; i += WD) has_s |= st.sup[i] > 0.0;
        for (int j = lane; j < nd; j += WD) has_d |= st.dem[j] > 0.0;
        if (!w.any(has_s) || !w.any(has_d)) break;
        if (it == EMD_MAX_AUGMENT) { ok = 0; break; }
        // ---- 2. Dijkstra from every source with supply left ----
        int cnt = 0;
        for (int i0 = 0; i0 < ns; i0 += WD) {
            const int i = i0 + lane;
            const bool root = i < ns && st.sup[i] > 0.0;
            const int p = w.prefix(root, cnt);
            if (i < ns) { st.ds[i] = root ? 0.0 : INF; st.pred_s[i] = -1; st.done_s[i] = root; }
            if (root) st.list[p] = i;
        }
        for (int j = lane; j < nd; j += WD) { st.dt[j] = INF; st.pred_t[j] = -1; st.done_t[j] = 0; }
        w.sync();
        int jstar = -1;
        double D = 0.0;
        for (;;) {
            // relax from the sources of st.list[0, cnt)
            for (int q = 0; q < cnt; ++q) {
                const int i = st.list[q];
                const double base = st.ds[i] + st.ps[i];
                const double* crow = st.cst + (long)i * nd;
                for (int j = lane; j < nd; j += WD) {
                    if (st.done_t[j]) continue;
                    const double v = base + crow[j] - st.pt[j];
                    if (v < st.dt[j]) { st.dt[j] = v; st.pred_t[j] = i; }
                }
            }
            // the nearest sink not yet settled
            double bd = INF;
            int bj = 0x7fffffff;
            for (int j = lane; j < nd; j += WD)
                if (!st.done_t[j] && emd_less(st.dt[j], j, bd, bj)) { bd = st.dt[j]; bj = j; }
            w.argmin(bd, bj);
            if (!(bd < INF)) break;                          // no path (non-finite costs): not converged
            w.sync();
            if (lane == 0) st.done_t[bj] = 1;
            if (st.dem[bj] > 0.0) { jstar = bj; D = bd; break; }
            // a settled sink without demand: its flow edges lead back (reduced cost 0) to sources at the same distance
            cnt = 0;
            for (int i0 = 0; i0 < ns; i0 += WD) {
                const int i = i0 + lane;
                const bool reach = i < ns && !st.done_s[i] && st.flw[(long)i * nd + bj] > 0.0;
                const int p = w.prefix(reach, cnt);
                if (reach) { st.ds[i] = bd; st.pred_s[i] = bj; st.done_s[i] = 1; st.list[p] = i; }
            }
            w.sync();
        }
        if (jstar < 0) { ok = 0; break; }
        // potentials: the labels, capped at the distance of the sink reached
        for (int i = lane; i < ns; i += WD) st.ps[i] += st.ds[i] < D ? st.ds[i] : D;
        for (int j = lane; j < nd; j += WD) st.pt[j] += st.dt[j] < D ? st.dt[j] : D;
        w.sync();
        // augment along the tree path by its bottleneck (an exhausted terminal / edge lands on exactly 0: x - x = 0)
        if (lane == 0) {
            double delta = st.dem[jstar];
            int j = jstar;
            for (int step = 0; step <= ns + nd; ++step) {
                const int i = st.pred_t[j];
                if (st.pred_s[i] < 0) { if (st.sup[i] < delta) delta = st.sup[i]; break; }
                const int j2 = st.pred_s[i];
                const double f = st.flw[(long)i * nd + j2];
                if (f < delta) delta = f;
                j = j2;
            }
            j = jstar;
            st.dem[j] -= delta;
            for (int step = 0; step <= ns + nd; ++step) {
                const int i = st.pred_t[j];
                st.flw[(long)i * nd + j] += delta;
                if (st.pred_s[i] < 0) { st.sup[i] -= delta; break; }
                const int j2 = st.pred_s[i];
                st.flw[(long)i * nd + j2] -= delta;
                j = j2;
            }
        }
        w.sync();
    }
    // cost of the flow, in a fixed order (per sink over the sources, then across lanes)
    double c = 0.0;
    for (int j = lane; j < nd; j += WD) {
        double cj = 0.0;
        for (int i = 0; i < ns; ++i) cj += st.flw[(long)i * nd + j] * st.cst[(long)i * nd + j];
        c += cj;
    }
    c = w.sum(c);
    *converged = ok;
    return c;
}

// pyemd.emd(P, Q, C) with the default penalty: transport + |sum P - sum Q| * max C.  Non-finite masses give NaN.
template <class W>
EMD_FN double emd_hat(const W& w, EmdState& st, const double* P, const double* Q, int n, const double* C, int* converged) {
    const int lane = w.lane(), WD = W::WIDTH;
    double sp = 0.0, sq = 0.0, cmax = 0.0;
    int bad = 0;
    for (int v = lane; v < n; v += WD) {
        sp += P[v]; sq += Q[v];
        bad |= !(P[v] - P[v] == 0.0) || !(Q[v] - Q[v] == 0.0);          // inf or NaN
    }
    for (long e = lane; e < (long)n * n; e += WD) cmax = C[e] > cmax ? C[e] : cmax;
    sp = w.sum(sp); sq = w.sum(sq); cmax = w.max(cmax);
    if (w.any(bad)) { *converged = 1; return __builtin_nan(""); }
    const double t = emd_transport(w, st, P, Q, n, C, converged);
    return t + (sp > sq ? sp - sq : sq - sp) * cmax;
}

}  // namespace sagen
