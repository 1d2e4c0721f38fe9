// Nested sampling by slice sampling in the whitened unit cube, pinned decision for decision.
//
// The loop runs where the live points are (vmx_nested_run, vegamx.hip: k_ns_iteration kills, whitens and starts the threads,
// k_ns_advance moves every thread's state machine by one likelihood answer and compacts the next requests);
// vega_amd/nested.py restates every expression below in NumPy (the `python` driver) and tests/helpers/nested_driver.cpp compiles
// this header with g++ so that tests/test_nested_host.py can hold the two against each other bit for bit (the boost part:
// tests/helpers/nested_boost_driver.cpp, tests/test_nested_boost_host.py; boost in a set: tests/helpers/nested_set_boost_driver.cpp).  No HIP type, no heap.
//
//   cube             the sampler works in u in [0, 1]^n; a physical parameter is lo + (hi - lo) u (map_cube), a uniform prior over
//                    the limits.  lnL = log_norm - 0.5 chi2 (vmx_ens::log_lik); a failed model (!vmx_ens::model_ok) has
//                    lnL = -inf and satisfies no constraint.
//   random numbers   vmx_ens::philox4x64_10 keyed (seed, stream).  Thread k at iteration t reads the blocks with counter
//                    (k, t, j, 1), j = 0, 1, 2 ... in the order it needs them (j: the thread's own draw index, so its stream
//                    depends on nothing but its own history); initial live point i reads (i, 0, j, 2), coordinate c from word
//                    c % 4 of block j = c / 4.  A uniform double from a word: vmx_ens::u01.
//   one iteration    nlive live points, K threads (1 <= K, nlive - K >= n + 1):
//     kill           rank_i = #{j : lnL_j < lnL_i, or lnL_j == lnL_i and j < i}; the points of rank 0 .. K-1 die in that order,
//                    death j recorded with the live count nlive - j; L* = lnL of rank K-1.
//     whiten         m = nlive - K survivors, sums over them in live-index order, one accumulator per entry:
//                    mean_a = (sum u_a) / m, cov_ab = (sum (u_a - mean_a)(u_b - mean_b)) / (m - 1), C its lower Cholesky factor
//                    (row by row, see cholesky); a pivot that is not positive makes the iteration use diag(sqrt(cov_aa)).
//     start          thread k copies survivor number vmx_ens::partner(word 0 of block 0, m) (survivors counted in live-index
//                    order); its draws go on at block 1.
//     slice steps    num_repeats times, under lnL > L* and inside the cube:
//                    direction  n + 1 words q = 0 .. n from the next n / 4 + 1 blocks (word q % 4 of block q / 4): g_q = 2 u - 1,
//                               d = C g / |g|; the last word is r.
//                    bracket    [L, R] = [-(r w), (1 - r) w] in units of d, w = 2.
//                    step out   L -= w while x + L d is acceptable, then R += w likewise (at most MAX_STEP_OUT times each).
//                    shrink     t = L + (R - L) u (word 0 of the next block); x + t d acceptable: the step ends there; otherwise
//                               the end on t's side moves to t (after MAX_SHRINK rejections the step ends where it began).
//                    a point outside the cube is unacceptable without an evaluation: the thread's request is then its own position
//                    and the answer is ignored.
//     replace        the K end points and their lnL take the killed points' slots, thread k the slot of rank k.
//
//   clustering       (optional: vmx_nested_run_clustered; off, everything above is what an iteration does) after the kill the m
//                    survivors, numbered by position in live-index order, are split into clusters and every cluster is whitened
//                    on its own:
//     distances      d2(i, j) = sum_a (u_ia - u_ja)^2 from 0.0 over a = 0 .. n-1 (dist2); neighbours are ordered by (d2, position)
//                    (nearer: duplicated live points occur, a slice step that gives up ends where it began); every survivor
//                    keeps its KNN = 8 nearest others (m - 1 if that is fewer; -1 fills the list).
//     components     at level k = 2 .. 8, i and j are linked when each is among the other's first k neighbours (link_level); c_k
//                    counts the connected components.  The first k >= 3 with c_k = c_{k-1} is used, otherwise k = 8.  A
//                    component's raw label is its smallest position.
//     clusters       a component of at least 2 n + 2 points is sizeable; the sizeable ones in the order (size descending, raw
//                    label ascending), at most MAX_CLUSTERS = 8, are the clusters; none: all survivors form one cluster.  Every
//                    other survivor joins the cluster of its nearest clustered survivor by (d2, position).
//     ids            live_cluster[nlive] (0: never labelled) and next_id (from 1) belong to the run's state.  The clusters in
//                    their order each take the most frequent non-zero previous id among their members (attached ones included),
//                    ties to the lowest id; none, or one an earlier cluster of this iteration took: next_id++.
//     factors        mean and covariance per cluster over its members in live-index order, divisor size - 1
//                    (cluster_mean_entry, cluster_cov_entry), then whiten, the diagonal fallback included.
//     threads        thread k walks with the factor of its start point's cluster; its end point inherits that cluster's id.
//     record         a death carries the id the point held when it was killed.
//
//   a set of runs    (vmx_nested_run_many; the functions at the end of this header, tests/helpers/nested_set_driver.cpp) E such
//                    runs, run e under the Philox key (seed, streams[e]), advanced together.  Nothing crosses runs except the
//                    row offsets: run e is the run above on its stream, the same functions in the same order.
//     phases         HEAD: the run's next iteration has to be headed (kill, whiten, start); WALK: some thread is asking; OUT: it
//                    has left the set.  The active list holds the runs not OUT in ascending run order (first_active,
//                    compact_active), the heading list those of them in HEAD, in the same order (heading_list).
//     status         GOING (0): the call's iterations are used up; STOPPED (1): the stop callback ended the run; NO_FINITE (2):
//                    with draw_live no live point has a finite lnL - the run is never entered (start_status).
//     a set round    the heading list is headed (skipped when empty); every thread of every active run takes the answer of the
//                    engine row it asked for last round and advances, and every run counts its requests; the requests are
//                    packed into the engine rows [0, total) in ascending (run, thread) order, run active[a] from row
//                    offset[a] = count[0] + ... + count[a - 1] (row_offsets: a sum in list order, no atomic decides a row); a run
//                    whose count is 0 has finished its iteration: its end points take the killed slots in the same round.  The
//                    host waits once, evaluates the rows when there are any, and for every run whose count was 0 adds one to
//                    its iterations done, asks its stop callback and moves it to OUT or HEAD (after_iteration); the others
//                    stay in WALK.  Runs do not wait for each other: a run whose iteration ended in round r is headed in
//                    round r + 1.  The iteration index of run e is iteration[e] + iterations_done[e], its record row
//                    iterations_done[e].
//     boost          (vmx_nested_run_many_phantoms) every run keeps its own phantom record by the rule of "boost" below, under its
//                    own stream: run e's kept points of a call lie in the rows [e capacity, e capacity + count[e]) of one record
//                    [E][capacity] (set_phantom_row), in the order that run accepted them, behind that run's own running count;
//                    a call needs capacity >= n_iterations K (num_repeats - 1) (set_phantom_capacity).  Nothing crosses runs.
//
//   boost            (optional: vmx_nested_run_phantoms; off, everything above is what a run does) the accepted points inside a
//                    thread's walk are kept beside the dead record instead of being thrown away - no likelihood row is spent.
//     phantom        thread k of iteration t has the phantom point r (1 <= r < num_repeats) when advance accepts a trial in
//                    S_SHRINK (T.inside != 0 && answer > L*) and T.repeat after the call is r < num_repeats (phantom_of, from the
//                    state and `inside` before the call and the thread after it).  The point is T.x, its lnL T.lnl = the answer,
//                    its birth contour the iteration's L*.  A step that gives up after MAX_SHRINK yields none, nor does the end
//                    point (r = num_repeats).
//     thinning       (k, t, r) is kept iff u01(word 0 of philox4x64_10(k, t, r, 3, seed, stream)) < f (phantom_kept), f in [0, 1]:
//                    the last counter word 3 is a domain of its own (threads 1, live points 2), so the run is the same run at any f.
//     record         per kept point u[n], lnL, birth, (iteration, thread, repeat), and with clustering the id of the thread's
//                    cluster (what its end point inherits); the canonical order is ascending (iteration, thread, repeat).
//
// Thread is a resumable state machine: advance(state, lnL of my last request) -> next request | done.  Every expression is the
// separately rounded IEEE operations written below (contraction off, as in vmx_ensemble.h); sqrt and / are correctly rounded.
#pragma once
#include "vmx_ensemble.h"

namespace vmx_ns {

constexpr int MAXN = 32;
constexpr int MAX_LIVE = 4096;
constexpr int MAX_STEP_OUT = 32;
constexpr int MAX_SHRINK = 64;
constexpr double WIDTH = 2.0;
enum State : int32_t { S_NEXT = 0, S_LEFT = 1, S_RIGHT = 2, S_SHRINK = 3, S_DONE = 4 };

struct Thread {
    double x[MAXN], d[MAXN], y[MAXN];       // position, direction, the point asked for (x + t d)
    double lnl, L, R, t;
    int64_t draw;                           // next block index of this thread in this iteration
    int32_t state, repeat, n_out, n_shrink, inside, reserved;
};

// what every thread of an iteration shares
struct Iteration {
    const double* C;                        // [n][n] lower factor
    double lstar;
    int64_t iteration;
    uint64_t seed, stream;
    int32_t n, num_repeats;
};

VMX_HD inline vmx_ens::Block thread_block(int64_t k, int64_t t, int64_t j, uint64_t seed, uint64_t stream)
{
    return vmx_ens::philox4x64_10((uint64_t)k, (uint64_t)t, (uint64_t)j, 1, seed, stream);
}

VMX_HD inline vmx_ens::Block live_block(int64_t i, int64_t j, uint64_t seed, uint64_t stream)
{
    return vmx_ens::philox4x64_10((uint64_t)i, 0, (uint64_t)j, 2, seed, stream);
}

// initial live point i: u[n]
VMX_HD inline void draw_live(int64_t i, int n, uint64_t seed, uint64_t stream, double* u)
{
    for (int c = 0; c < n; c += 4) {
        const vmx_ens::Block b = live_block(i, c / 4, seed, stream);
        for (int q = 0; q < 4 && c + q < n; ++q) u[c + q] = vmx_ens::u01(b.w[q]);
    }
}

VMX_HD inline double map_cube(double lo, double hi, double u)
{
    VMX_NO_CONTRACT
    const double w = hi - lo;
    const double p = w * u;
    return lo + p;
}

VMX_HD inline double lnl_of(int32_t status, double chi2, double log_norm)
{
    return vmx_ens::model_ok(status, chi2) ? vmx_ens::log_lik(log_norm, chi2) : -INFINITY;
}

// ---- kill
VMX_HD inline int rank_of(int i, const double* lnl, int nlive)
{
    const double v = lnl[i];
    int r = 0;
    for (int j = 0; j < nlive; ++j) r += (lnl[j] < v || (lnl[j] == v && j < i)) ? 1 : 0;
    return r;
}

// ---- whiten (rank[i] >= K: a survivor)
VMX_HD inline double mean_entry(int a, const double* u, const int32_t* rank, int nlive, int K, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    for (int i = 0; i < nlive; ++i)
        if (rank[i] >= K) acc = acc + u[(size_t)i * n + a];
    return acc / (double)(nlive - K);
}

VMX_HD inline double cov_entry(int a, int b, const double* u, const int32_t* rank, const double* mean, int nlive, int K, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    const double ma = mean[a], mb = mean[b];
    for (int i = 0; i < nlive; ++i) {
        if (rank[i] < K) continue;
        const double da = u[(size_t)i * n + a] - ma;
        const double db = u[(size_t)i * n + b] - mb;
        const double p = da * db;
        acc = acc + p;
    }
    return acc / (double)(nlive - K - 1);
}

// lower Cholesky factor of cov [n][n] (its lower triangle is read) into C [n][n], column by column; false: a pivot was not positive
VMX_HD inline bool cholesky(int n, const double* cov, double* C)
{
    VMX_NO_CONTRACT
    for (int i = 0; i < n * n; ++i) C[i] = 0.0;
    for (int j = 0; j < n; ++j) {
        double s = cov[j * n + j];
        for (int k = 0; k < j; ++k) {
            const double p = C[j * n + k] * C[j * n + k];
            s = s - p;
        }
        if (!(s > 0.0)) return false;
        const double piv = sqrt(s);
        C[j * n + j] = piv;
        for (int i = j + 1; i < n; ++i) {
            double t = cov[i * n + j];
            for (int k = 0; k < j; ++k) {
                const double p = C[i * n + k] * C[j * n + k];
                t = t - p;
            }
            C[i * n + j] = t / piv;
        }
    }
    return true;
}

// the factor an iteration uses; true: the Cholesky factor, false: the diagonal of standard deviations
VMX_HD inline bool whiten(int n, const double* cov, double* C)
{
    if (cholesky(n, cov, C)) return true;
    for (int i = 0; i < n * n; ++i) C[i] = 0.0;
    for (int a = 0; a < n; ++a) C[a * n + a] = cov[a * n + a] > 0.0 ? sqrt(cov[a * n + a]) : 0.0;
    return false;
}

// ---- the thread
// survivor number (in live-index order) that thread k of iteration t starts from
VMX_HD inline int64_t start_choice(int64_t k, int64_t t, int64_t m, uint64_t seed, uint64_t stream)
{
    return vmx_ens::partner(thread_block(k, t, 0, seed, stream).w[0], m);
}

VMX_HD inline void start(Thread& T, int n, const double* u, double lnl)
{
    for (int i = 0; i < n; ++i) { T.x[i] = u[i]; T.y[i] = u[i]; T.d[i] = 0.0; }
    T.lnl = lnl; T.L = 0.0; T.R = 0.0; T.t = 0.0;
    T.draw = 1;
    T.state = S_NEXT; T.repeat = 0; T.n_out = 0; T.n_shrink = 0; T.inside = 1; T.reserved = 0;
}

// y = x + t d, and whether it lies in the cube
VMX_HD inline void trial(Thread& T, int n)
{
    VMX_NO_CONTRACT
    bool in = true;
    for (int i = 0; i < n; ++i) {
        const double p = T.t * T.d[i];
        const double v = T.x[i] + p;
        T.y[i] = v;
        in = in && v >= 0.0 && v <= 1.0;
    }
    T.inside = in ? 1 : 0;
}

VMX_HD inline void new_direction(Thread& T, const Iteration& I, int64_t k)
{
    VMX_NO_CONTRACT
    const int n = I.n;
    double g[MAXN];
    double r = 0.0;
    for (int q = 0; q <= n; q += 4) {
        const vmx_ens::Block b = thread_block(k, I.iteration, T.draw + q / 4, I.seed, I.stream);
        for (int w = 0; w < 4 && q + w <= n; ++w) {
            const double u = vmx_ens::u01(b.w[w]);
            if (q + w < n) { const double two = 2.0 * u; g[q + w] = two - 1.0; }
            else r = u;
        }
    }
    T.draw += n / 4 + 1;
    double s = 0.0;
    for (int i = 0; i < n; ++i) { const double p = g[i] * g[i]; s = s + p; }
    double nrm = sqrt(s);
    if (!(nrm > 0.0)) { g[0] = 1.0; nrm = 1.0; }
    for (int i = 0; i < n; ++i) g[i] = g[i] / nrm;
    for (int i = 0; i < n; ++i) {
        double acc = 0.0;
        for (int j = 0; j <= i; ++j) { const double p = I.C[i * n + j] * g[j]; acc = acc + p; }
        T.d[i] = acc;
    }
    const double rw = r * WIDTH;
    T.L = -rw;
    const double q1 = 1.0 - r;
    T.R = q1 * WIDTH;
}

VMX_HD inline void draw_trial(Thread& T, const Iteration& I, int64_t k)
{
    VMX_NO_CONTRACT
    const double u = vmx_ens::u01(thread_block(k, I.iteration, T.draw, I.seed, I.stream).w[0]);
    T.draw += 1;
    const double wid = T.R - T.L;
    const double p = wid * u;
    T.t = T.L + p;
    trial(T, I.n);
}

// `answer`: lnL of the thread's last request (ignored in S_NEXT, and whenever that request lay outside the cube).
// true: T.y / T.inside hold the next request (the thread asks for T.inside ? T.y : T.x); false: the thread is done, T.x / T.lnl
// are its end point.
VMX_HD inline bool advance(Thread& T, const Iteration& I, int64_t k, double answer)
{
    VMX_NO_CONTRACT
    const bool ok = T.inside != 0 && answer > I.lstar;
    if (T.state == S_LEFT) {
        if (ok && T.n_out < MAX_STEP_OUT) { T.L = T.L - WIDTH; T.n_out += 1; T.t = T.L; trial(T, I.n); return true; }
        T.state = S_RIGHT; T.n_out = 0; T.t = T.R; trial(T, I.n);
        return true;
    }
    if (T.state == S_RIGHT) {
        if (ok && T.n_out < MAX_STEP_OUT) { T.R = T.R + WIDTH; T.n_out += 1; T.t = T.R; trial(T, I.n); return true; }
        T.state = S_SHRINK; T.n_shrink = 0;
        draw_trial(T, I, k);
        return true;
    }
    if (T.state == S_SHRINK) {
        if (ok) {
            for (int i = 0; i < I.n; ++i) T.x[i] = T.y[i];
            T.lnl = answer; T.repeat += 1; T.state = S_NEXT;
        } else {
            if (T.t < 0.0) T.L = T.t; else T.R = T.t;
            T.n_shrink += 1;
            if (T.n_shrink < MAX_SHRINK) { draw_trial(T, I, k); return true; }
            T.repeat += 1; T.state = S_NEXT;
        }
    }
    if (T.state == S_NEXT) {
        if (T.repeat >= I.num_repeats) { T.state = S_DONE; T.inside = 1; return false; }
        new_direction(T, I, k);
        T.state = S_LEFT; T.n_out = 0; T.t = T.L;
        trial(T, I.n);
        return true;
    }
    return false;
}

// ---- boost: the accepted points inside a walk (nothing here changes advance or a thread's stream)
// the index r of the phantom point the last call of advance produced, 0: none.  `state_before` / `inside_before`: T.state and
// T.inside when advance was called with `answer`; T: the thread after the call.
VMX_HD inline int32_t phantom_of(int32_t state_before, int32_t inside_before, double answer, double lstar, const Thread& T,
                                 int32_t num_repeats)
{
    const bool accepted = state_before == S_SHRINK && inside_before != 0 && answer > lstar;
    return accepted && T.repeat < num_repeats ? T.repeat : 0;
}

// whether the phantom point r of thread k at iteration t is kept at the fraction f
VMX_HD inline bool phantom_kept(int64_t k, int64_t t, int32_t r, double f, uint64_t seed, uint64_t stream)
{
    return vmx_ens::u01(vmx_ens::philox4x64_10((uint64_t)k, (uint64_t)t, (uint64_t)r, 3, seed, stream).w[0]) < f;
}

// ---- clustering of the survivors (positions 0 .. m-1; `surv` maps a position to its row of u and of prev_id, nullptr: itself)
constexpr int KNN = 8;
constexpr int MAX_CLUSTERS = 8;
constexpr int32_t NO_NEIGHBOUR = 0x7fffffff;

VMX_HD inline int row_of(const int32_t* surv, int p) { return surv ? surv[p] : p; }

VMX_HD inline double dist2(const double* a, const double* b, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    for (int c = 0; c < n; ++c) {
        const double d = a[c] - b[c];
        const double p = d * d;
        acc = acc + p;
    }
    return acc;
}

VMX_HD inline bool nearer(double d, int32_t p, double d_than, int32_t p_than) { return d < d_than || (d == d_than && p < p_than); }

// the sorted list (d[KNN], p[KNN]; empty places: +inf, NO_NEIGHBOUR) after the candidate (cd, cp) has been offered to it
VMX_HD inline void nn_insert(double* d, int32_t* p, double cd, int32_t cp)
{
    if (!nearer(cd, cp, d[KNN - 1], p[KNN - 1])) return;
    for (int s = 0; s < KNN; ++s) {
        const bool in = nearer(cd, cp, d[s], p[s]);
        const double kd = in ? cd : d[s], od = in ? d[s] : cd;
        const int32_t kp = in ? cp : p[s], op = in ? p[s] : cp;
        d[s] = kd; p[s] = kp; cd = od; cp = op;
    }
}

// the neighbours of survivor i into out[KNN]
VMX_HD inline void knn_of(int i, const double* u, const int32_t* surv, int m, int n, int32_t* out)
{
    double d[KNN];
    int32_t p[KNN];
    for (int s = 0; s < KNN; ++s) { d[s] = INFINITY; p[s] = NO_NEIGHBOUR; }
    const double* x = u + (size_t)row_of(surv, i) * n;
    for (int j = 0; j < m; ++j)
        if (j != i) nn_insert(d, p, dist2(x, u + (size_t)row_of(surv, j) * n, n), j);
    for (int s = 0; s < KNN; ++s) out[s] = p[s] == NO_NEIGHBOUR ? -1 : p[s];
}

// the smallest level k at which i and its q-th neighbour are linked (each among the other's first k); KNN + 1: at none
VMX_HD inline int link_level(const int32_t* nn, int i, int q)
{
    const int j = nn[(size_t)i * KNN + q];
    if (j < 0) return KNN + 1;
    for (int r = 0; r < KNN; ++r)
        if (nn[(size_t)j * KNN + r] == i) return (q > r ? q : r) + 1;
    return KNN + 1;
}

// one sweep of min-label propagation over the links of level <= k; true: a label changed
VMX_HD inline bool propagate(const int32_t* nn, int m, int k, int32_t* label)
{
    bool changed = false;
    for (int i = 0; i < m; ++i)
        for (int q = 0; q < k; ++q) {
            if (link_level(nn, i, q) > k) continue;
            const int32_t l = label[nn[(size_t)i * KNN + q]];
            if (l < label[i]) { label[i] = l; changed = true; }
        }
    return changed;
}

// the key by which a cluster picks its id among its members' previous ones: more members first, then the lower id
VMX_HD inline uint64_t id_key(int32_t count, int32_t id) { return ((uint64_t)(uint32_t)count << 32) | (uint32_t)(0x7fffffff - id); }
VMX_HD inline int32_t id_of_key(uint64_t key) { return key ? 0x7fffffff - (int32_t)(uint32_t)(key & 0xffffffffu) : 0; }

// the clusters' ids in their order from the best key of each (0: no member had an id)
VMX_HD inline void assign_ids(int n_clusters, const uint64_t* best, int32_t* next_id, int32_t* cluster_id)
{
    for (int c = 0; c < n_clusters; ++c) {
        int32_t id = id_of_key(best[c]);
        for (int e = 0; e < c; ++e)
            if (cluster_id[e] == id) id = 0;
        if (id == 0) { id = *next_id; *next_id += 1; }
        cluster_id[c] = id;
    }
}

// Distances to ids, serially: nn [m][KNN], label / size / slot0 [m] are the caller's scratch; slot [m] the cluster of every
// survivor (its place in the order), cluster_id / cluster_size [MAX_CLUSTERS], *k_used, *n_clusters; *next_id moves on.
VMX_HD inline void cluster_points(const double* u, const int32_t* surv, int m, int n, const int32_t* prev_id, int32_t* next_id,
                                  int32_t* nn, int32_t* label, int32_t* size, int32_t* slot0, int32_t* slot, int32_t* cluster_id,
                                  int32_t* cluster_size, int32_t* k_used, int32_t* n_clusters)
{
    for (int i = 0; i < m; ++i) knn_of(i, u, surv, m, n, nn + (size_t)i * KNN);
    for (int i = 0; i < m; ++i) label[i] = i;
    int k = 2, before = 0;
    for (;; ++k) {
        for (int sweep = 0; sweep < m && propagate(nn, m, k, label); ++sweep) {}
        int count = 0;
        for (int i = 0; i < m; ++i) count += label[i] == i ? 1 : 0;
        if ((k >= 3 && count == before) || k == KNN) break;
        before = count;
    }
    *k_used = k;
    for (int i = 0; i < m; ++i) size[i] = 0;
    for (int i = 0; i < m; ++i) size[label[i]] += 1;
    int nc = 0;
    int32_t root[MAX_CLUSTERS];
    for (; nc < MAX_CLUSTERS; ++nc) {
        int best = -1;
        for (int r = 0; r < m; ++r) {
            if (label[r] != r || size[r] < 2 * n + 2) continue;
            bool taken = false;
            for (int e = 0; e < nc; ++e) taken = taken || root[e] == r;
            if (!taken && (best < 0 || size[r] > size[best])) best = r;
        }
        if (best < 0) break;
        root[nc] = best;
    }
    if (nc == 0) {
        for (int i = 0; i < m; ++i) { slot0[i] = 0; slot[i] = 0; }
        nc = 1;
    } else {
        for (int i = 0; i < m; ++i) {
            slot0[i] = -1;
            for (int c = 0; c < nc; ++c)
                if (label[i] == root[c]) slot0[i] = c;
        }
        for (int i = 0; i < m; ++i) {
            slot[i] = slot0[i];
            if (slot0[i] >= 0) continue;
            const double* x = u + (size_t)row_of(surv, i) * n;
            double bd = INFINITY;
            int32_t bp = NO_NEIGHBOUR;
            for (int j = 0; j < m; ++j) {
                if (slot0[j] < 0) continue;
                const double d = dist2(x, u + (size_t)row_of(surv, j) * n, n);
                if (nearer(d, j, bd, bp)) { bd = d; bp = j; }
            }
            slot[i] = slot0[bp];
        }
    }
    *n_clusters = nc;
    uint64_t best[MAX_CLUSTERS];
    for (int c = 0; c < MAX_CLUSTERS; ++c) { cluster_size[c] = 0; cluster_id[c] = 0; best[c] = 0; }
    for (int i = 0; i < m; ++i) {
        cluster_size[slot[i]] += 1;
        const int32_t id = prev_id[row_of(surv, i)];
        if (id == 0) continue;
        int32_t count = 0;
        for (int j = 0; j < m; ++j) count += (slot[j] == slot[i] && prev_id[row_of(surv, j)] == id) ? 1 : 0;
        const uint64_t key = id_key(count, id);
        if (key > best[slot[i]]) best[slot[i]] = key;
    }
    assign_ids(nc, best, next_id, cluster_id);
}

// mean and covariance of cluster c (size members) over its members in order, one accumulator per entry
VMX_HD inline double cluster_mean_entry(int a, const double* u, const int32_t* surv, const int32_t* slot, int m, int c, int size, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    for (int i = 0; i < m; ++i)
        if (slot[i] == c) acc = acc + u[(size_t)row_of(surv, i) * n + a];
    return acc / (double)size;
}

VMX_HD inline double cluster_cov_entry(int a, int b, const double* u, const int32_t* surv, const int32_t* slot, const double* mean,
                                       int m, int c, int size, int n)
{
    VMX_NO_CONTRACT
    double acc = 0.0;
    const double ma = mean[a], mb = mean[b];
    for (int i = 0; i < m; ++i) {
        if (slot[i] != c) continue;
        const double* x = u + (size_t)row_of(surv, i) * n;
        const double da = x[a] - ma;
        const double db = x[b] - mb;
        const double p = da * db;
        acc = acc + p;
    }
    return acc / (double)(size - 1);
}

// ---- a set of runs (vmx_nested_run_many): E independent runs advanced together; nothing below crosses runs but row_offsets
constexpr int32_t HEAD = 0, WALK = 1, OUT = 2;
constexpr int32_t GOING = 0, STOPPED = 1, NO_FINITE = 2;

// after the draw: `finite` of the nlive drawn points have a finite lnL
VMX_HD inline int32_t start_status(int64_t finite) { return finite > 0 ? GOING : NO_FINITE; }

// the runs a call begins with, in ascending order: those with status GOING when there is an iteration to do; they are in HEAD,
// the others OUT.  Returns their number.
VMX_HD inline int first_active(const int32_t* status, int E, int64_t n_iterations, int32_t* active, int32_t* phase)
{
    int A = 0;
    for (int e = 0; e < E; ++e) {
        phase[e] = status[e] == GOING && n_iterations > 0 ? HEAD : OUT;
        if (phase[e] != OUT) active[A++] = e;
    }
    return A;
}

// the active runs whose next iteration has to be headed, in the list's order.  Returns their number.
VMX_HD inline int heading_list(const int32_t* active, int A, const int32_t* phase, int32_t* heading)
{
    int H = 0;
    for (int a = 0; a < A; ++a)
        if (phase[active[a]] == HEAD) heading[H++] = active[a];
    return H;
}

// the first engine row of every active run from the runs' request counts, summed in list order.  Returns the total.
VMX_HD inline int64_t row_offsets(const int32_t* count, int A, int64_t* offset)
{
    int64_t total = 0;
    for (int a = 0; a < A; ++a) { offset[a] = total; total += count[a]; }
    return total;
}

// the phase of a run after a round in which it asked for `count` rows: 0 ends its iteration (the host decides: after_iteration)
VMX_HD inline bool iteration_ended(int32_t count) { return count == 0; }

// the phase of a run whose iteration has just ended, `done` iterations into a call of n_iterations; *status moves to STOPPED
// when its stop callback said so
VMX_HD inline int32_t after_iteration(bool stopped, int64_t done, int64_t n_iterations, int32_t* status)
{
    if (stopped) { *status = STOPPED; return OUT; }
    return done >= n_iterations ? OUT : HEAD;
}

// drop the runs that are OUT; the rest keep their (ascending) order and move up.  Returns the new number.
VMX_HD inline int compact_active(int32_t* active, int A, const int32_t* phase)
{
    int B = 0;
    for (int a = 0; a < A; ++a)
        if (phase[active[a]] != OUT) active[B++] = active[a];
    return B;
}

// boost in a set: the rows a call's phantom record needs per run (what one run can keep at the most) ...
VMX_HD inline int64_t set_phantom_capacity(int64_t n_iterations, int64_t K, int64_t num_repeats)
{
    return n_iterations * K * (num_repeats - 1);
}

// ... and the row of the record [E][capacity] that holds the p-th point a round adds behind the `count` rows `run` has written
VMX_HD inline int64_t set_phantom_row(int64_t run, int64_t capacity, int64_t count, int64_t p) { return run * capacity + count + p; }

}  // namespace vmx_ns
