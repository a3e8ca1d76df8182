// poisson_kernels.hip -- gravity.gravity_type = "PoissonGrav" on a level, 3-D Cartesian, Dirichlet on every edge of the level.
// ONE set of multigrid passes, each a template over what it has to know about the edge of the level, instantiated twice:
// MgOneBox (the level is one box; profiler names k_mg_*, k_grad_phi) and MgBoxes (a refined level of SEVERAL boxes: one array
// over their bounding box, a byte of coverage flags per zone and an array of face values; profiler names k_mgb_*)
//   k_mg_rhs, k_mgb_rhs                   b = (4 pi G) * rho, from one FAB / from the boxes' own FABs
//   k_mg_smooth, k_mg_bottom              red-black Gauss-Seidel on one level; the bottom solve is the same sweep, all of them
//                                         in one launch of one workgroup
//   k_mg_residual, k_mg_restrict, k_mg_prolong, k_mg_norm_partial + k_mg_norm_final
//                                         the other four passes of the V-cycle
//   k_grad_phi, k_mgb_grad                g = -grad(phi) on the valid zones (Gravity.cpp:874-878 over MLMG's getGradSolution)
//   k_mp_partial + k_mp_final             the multipole moments of Gravity::fill_multipole_BCs (Gravity.cpp:1742-2032, multipole_add
//                                         of Gravity_util.H) with boundary_only = 1: every zone falls in the last radial bin
//   k_mp_phi_bc                           the boundary potential (Gravity.cpp:2066-2216) on the zones of a FAB outside the domain
//   k_phi_cf_bc, k_phi_cf_boxes           the coarse-fine boundary potential of a refined level's own solve (the end of the file),
//                                         into the ghost zones of phi / into the face array of a union of boxes
// The multigrid is AMReX's [3P]: its arithmetic is not in the reference tree and is not pinned.  It is
// written so that a restatement with the same order of operations reproduces the `exact` build bit for bit: the header comment
// of every pass gives that order, and the passes hold no transcendental.  The `contract` build fuses these passes' multiply-adds.
// The multipole kernels (the second half of the file) are compiled without contraction in BOTH builds: their terms go through
// pow / atan2 / sin / cos, whose arguments must be the restatement's bits for a per-call allowance to mean anything (the Makefile
// gives this file -ffp-contract=fast-honor-pragmas in the `contract` build, so that the pragma in front of them holds).
// No floating-point atomics anywhere: the moments are summed in two stages in an order fixed by the box table (the same bits on
// every call; across streams as long as the host orders the calls of a context, which has one workspace), the norm is a
// maximum.  A zone centred exactly on the multipole centre has r = 0 and cosTheta = 0 / 0, here as in Gravity.cpp:1917: NaN
// moments for l >= 1 (include/castro_hydro_amd.h).  Everything runs on the caller's stream; the solve reads one norm back per V-cycle.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../include/castro_hydro_amd.h"
#include "hydro_device.h"
#include "ctu_kernels.h"

namespace cad {

constexpr int MG_WG = 256;
constexpr int MG_BOTTOM_WG = 1024;
constexpr int MG_NORM_MAX_WG = 1024;

__device__ __forceinline__ long mg_at(const DFab& F, int i, int j, int k)
{
    return (long)(i - F.lo[0]) + F.sy * (long)(j - F.lo[1]) + F.sz * (long)(k - F.lo[2]);
}

// thread q of a colour launch -> the zone (ii, jj, kk) of that colour, relative to the level's box: the row (jj, kk) is cut into
// x-pairs (2 ip, 2 ip + 1) and the thread takes the one with (ii + jj + kk) & 1 == colour.  false: no such zone
__device__ __forceinline__ bool mg_colour_zone(long q, const MgLevel& L, int colour, int& ii, int& jj, int& kk)
{
    const int npair = (L.n[0] + 1) >> 1;
    const int ip = (int)(q % npair);
    const long r = q / npair;
    jj = (int)(r % L.n[1]);
    kk = (int)(r / L.n[1]);
    ii = 2 * ip + ((jj + kk + colour) & 1);
    return ii < L.n[0];
}

// zone q of the box of L, x fastest, relative to its low corner
__device__ __forceinline__ void mg_zone(long q, const MgLevel& L, int& ii, int& jj, int& kk)
{
    ii = (int)(q % L.n[0]);
    const long rr = q / L.n[0];
    jj = (int)(rr % L.n[1]);
    kk = (int)(rr / L.n[1]);
}

__device__ __forceinline__ long mg_flag_at(const MgLevel& L, int ii, int jj, int kk)
{
    return (long)ii + (long)L.n[0] * ((long)jj + (long)L.n[1] * kk);
}

// the value on the (d, side) face of the zone (i, j, k): the low d-face of the zone (i, j, k) + side * e_d
__device__ __forceinline__ double mgb_face_value(const DFab& X, int d, int side, int i, int j, int k)
{
    if (!X.p) return 0.0;
    return X.p[mg_at(X, i + (d == 0 ? side : 0), j + (d == 1 ? side : 0), k + (d == 2 ? side : 0)) + X.sn * d];
}

// ---- the edge of a level ------------------------------------------------------------------------------------------------------
// A pass asks two questions of the level it runs on: is this zone part of the level, and is this face of the zone an edge of the
// level -- and if so, which value sits ON it.  The two sets of answers:
//   MgOneBox  the level is the box L.  Every zone is part of it, a face is an edge where the zone is the first or the last of its
//             row, and the value on it is the neighbour the pass has loaded: the ghost zone of phi, which holds phi ON the face
//             (level 0) or 0 (the coarser levels, whose ghost zones stay zero).  All of it is known when the pass is compiled
//   MgBoxes   the level is a union of boxes inside L, the bounding box >> m; colours are relative to its low corner.  A byte of
//             flags per zone of L, made on the host (MGF_*), says "covered" and "the neighbour across this face is not covered",
//             and the value ON such a face is read from the face array X of level 0 -- an uncovered zone at a concave corner of
//             the union is the neighbour of two covered zones across two faces with two values, so it cannot hold them -- or is
//             0.0 on the coarser levels (X.p == nullptr).  Zones that are not covered are never written
// zone(q) loads what the other queries are asked with (q: mg_flag_at).  The passes that ask the first question only take the base
// types.  As kernel arguments the types are laid out as (L) and (L, flags, X).
struct MgWhole {
    MgLevel L;
    __device__ unsigned zone(long) const { return 0u; }
    static __device__ bool covered(unsigned) { return true; }
};
struct MgMasked {
    MgLevel L;
    const unsigned char* __restrict__ flags;
    __device__ unsigned zone(long q) const { return flags[q]; }
    static __device__ bool covered(unsigned fl) { return fl & MGF_COVERED; }
};
struct MgOneBox : MgWhole {
    static __device__ bool any_edge(unsigned) { return true; }
    __device__ bool edge(unsigned, const int rel[3], int d, int side) const { return rel[d] == (side ? L.n[d] - 1 : 0); }
    __device__ double on_edge(int, int, int, int, int, double neighbour) const { return neighbour; }
};
struct MgBoxes : MgMasked {
    DFab X;
    static __device__ bool any_edge(unsigned fl) { return fl & ~MGF_COVERED; }
    __device__ bool edge(unsigned fl, const int[3], int d, int side) const { return fl & mgf_face(d, side); }
    __device__ double on_edge(int d, int side, int i, int j, int k, double) const { return mgb_face_value(X, d, side, i, j, k); }
};

// The smoother, one zone.  With p the zone's value, the six neighbours xm, xp, ym, yp, zm, zp and the right-hand side b:
//   a neighbour across an edge of the level is replaced by 2.0 * f, f the value ON the face; the - p of the linear ghost
//   2 f - p goes to the diagonal:
//   dg = cdiag; if (low x face) dg = dg + cx; if (high x face) dg = dg + cx; then y, then z (cdiag = 2.0 * ((cx + cy) + cz),
//   cx = 1.0 / (hx * hx), ... formed on the host)
//   p = (((cx * (xm + xp) + cy * (ym + yp)) + cz * (zm + zp)) - b) / dg
template <class E>
__device__ __forceinline__ double mg_relax(const DFab& P, const DFab& B, const E& e, unsigned fl, int ii, int jj, int kk)
{
    const MgLevel& L = e.L;
    const int i = L.lo[0] + ii, j = L.lo[1] + jj, k = L.lo[2] + kk, rel[3] = { ii, jj, kk };
    const double* p = P.p + mg_at(P, i, j, k);
    double xm = p[-1], xp = p[1], ym = p[-P.sy], yp = p[P.sy], zm = p[-P.sz], zp = p[P.sz];
    double dg = L.cdiag;
    if (E::any_edge(fl)) {
        if (e.edge(fl, rel, 0, 0)) { xm = 2.0 * e.on_edge(0, 0, i, j, k, xm); dg = dg + L.cx; }
        if (e.edge(fl, rel, 0, 1)) { xp = 2.0 * e.on_edge(0, 1, i, j, k, xp); dg = dg + L.cx; }
        if (e.edge(fl, rel, 1, 0)) { ym = 2.0 * e.on_edge(1, 0, i, j, k, ym); dg = dg + L.cy; }
        if (e.edge(fl, rel, 1, 1)) { yp = 2.0 * e.on_edge(1, 1, i, j, k, yp); dg = dg + L.cy; }
        if (e.edge(fl, rel, 2, 0)) { zm = 2.0 * e.on_edge(2, 0, i, j, k, zm); dg = dg + L.cz; }
        if (e.edge(fl, rel, 2, 1)) { zp = 2.0 * e.on_edge(2, 1, i, j, k, zp); dg = dg + L.cz; }
    }
    const double b = B.p[mg_at(B, i, j, k)];
    const double off = (L.cx * (xm + xp) + L.cy * (ym + yp)) + L.cz * (zm + zp);
    return (off - b) / dg;
}

// thread q of a sweep of one colour: its zone, where the level has one, is replaced by mg_relax of its neighbours
template <class E>
__device__ __forceinline__ void mg_sweep_zone(const DFab& P, const DFab& B, const E& e, long q, int colour)
{
    int ii, jj, kk;
    if (!mg_colour_zone(q, e.L, colour, ii, jj, kk)) return;
    const unsigned fl = e.zone(mg_flag_at(e.L, ii, jj, kk));
    if (!E::covered(fl)) return;
    const double v = mg_relax(P, B, e, fl, ii, jj, kk);
    P.p[mg_at(P, e.L.lo[0] + ii, e.L.lo[1] + jj, e.L.lo[2] + kk)] = v;
}

// One sweep of one colour: every zone of that colour is replaced by mg_relax of its neighbours, which are all of the other
// colour -- the order of the zones within the sweep does not matter
template <class E>
__global__ void __launch_bounds__(MG_WG) k_mg_smooth(DFab P, DFab B, E e, int colour)
{
    const long q = (long)blockIdx.x * MG_WG + threadIdx.x;
    const int npair = (e.L.n[0] + 1) >> 1;
    if (q >= (long)npair * e.L.n[1] * e.L.n[2]) return;
    mg_sweep_zone(P, B, e, q, colour);
}

// The bottom solve: `sweeps` times colour 0, then colour 1, of k_mg_smooth's arithmetic by ONE workgroup (the coarsest level holds
// at most CASTRO_AMD_POISSON_MAX_BOTTOM zones of its box); a barrier separates the colours
template <class E>
__global__ void __launch_bounds__(MG_BOTTOM_WG) k_mg_bottom(DFab P, DFab B, E e, int sweeps)
{
    const int npair = (e.L.n[0] + 1) >> 1;
    const long nq = (long)npair * e.L.n[1] * e.L.n[2];
    for (int s = 0; s < sweeps; ++s) {
        for (int colour = 0; colour < 2; ++colour) {
            for (long q = threadIdx.x; q < nq; q += MG_BOTTOM_WG) mg_sweep_zone(P, B, e, q, colour);
            __syncthreads();
        }
    }
}

// The residual.  A neighbour across an edge of the level is the linear ghost 2.0 * f - p, f the value ON the face;
//   lap = (cx * ((xm + xp) - 2.0 * p) + cy * ((ym + yp) - 2.0 * p)) + cz * ((zm + zp) - 2.0 * p);   r = b - lap
template <class E>
__global__ void __launch_bounds__(MG_WG) k_mg_residual(DFab P, DFab B, DFab R, E e)
{
    const MgLevel& L = e.L;
    const long q = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (q >= (long)L.n[0] * L.n[1] * L.n[2]) return;
    const unsigned fl = e.zone(q);
    if (!E::covered(fl)) return;
    int rel[3];
    mg_zone(q, L, rel[0], rel[1], rel[2]);
    const int i = L.lo[0] + rel[0], j = L.lo[1] + rel[1], k = L.lo[2] + rel[2];
    const double* p = P.p + mg_at(P, i, j, k);
    const double pc = p[0];
    double xm = p[-1], xp = p[1], ym = p[-P.sy], yp = p[P.sy], zm = p[-P.sz], zp = p[P.sz];
    if (E::any_edge(fl)) {
        if (e.edge(fl, rel, 0, 0)) xm = 2.0 * e.on_edge(0, 0, i, j, k, xm) - pc;
        if (e.edge(fl, rel, 0, 1)) xp = 2.0 * e.on_edge(0, 1, i, j, k, xp) - pc;
        if (e.edge(fl, rel, 1, 0)) ym = 2.0 * e.on_edge(1, 0, i, j, k, ym) - pc;
        if (e.edge(fl, rel, 1, 1)) yp = 2.0 * e.on_edge(1, 1, i, j, k, yp) - pc;
        if (e.edge(fl, rel, 2, 0)) zm = 2.0 * e.on_edge(2, 0, i, j, k, zm) - pc;
        if (e.edge(fl, rel, 2, 1)) zp = 2.0 * e.on_edge(2, 1, i, j, k, zp) - pc;
    }
    const double tp = 2.0 * pc;
    const double lap = (L.cx * ((xm + xp) - tp) + L.cy * ((ym + yp) - tp)) + L.cz * ((zm + zp) - tp);
    R.p[mg_at(R, i, j, k)] = B.p[mg_at(B, i, j, k)] - lap;
}

// The restriction onto the coarse zone (I, J, K) of the level c (the COARSE one; its children are 2 I + a, 2 J + b, 2 K + c
// relative to the fine box, whose low corner is flo, and the 8 children of a zone of the level are all zones of the fine
// level): with r_abc the children's residuals,
//   b_c = (((((((r000 + r100) + r010) + r110) + r001) + r101) + r011) + r111) * 0.125
// and the coarse correction starts from zero: phi_c = 0
template <class C>
__global__ void __launch_bounds__(MG_WG) k_mg_restrict(DFab RF, int flo0, int flo1, int flo2, DFab BC, DFab PC, C c)
{
    const MgLevel& L = c.L;
    const long q = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (q >= (long)L.n[0] * L.n[1] * L.n[2]) return;
    if (!C::covered(c.zone(q))) return;
    int ii, jj, kk;
    mg_zone(q, L, ii, jj, kk);
    const double* r = RF.p + mg_at(RF, flo0 + 2 * ii, flo1 + 2 * jj, flo2 + 2 * kk);
    double s = r[0] + r[1];
    s = s + r[RF.sy];
    s = s + r[RF.sy + 1];
    s = s + r[RF.sz];
    s = s + r[RF.sz + 1];
    s = s + r[RF.sz + RF.sy];
    s = s + r[RF.sz + RF.sy + 1];
    const int i = L.lo[0] + ii, j = L.lo[1] + jj, k = L.lo[2] + kk;
    BC.p[mg_at(BC, i, j, k)] = s * 0.125;
    PC.p[mg_at(PC, i, j, k)] = 0.0;
}

// The prolongation onto the fine zone (ii, jj, kk) of the level f (the FINE one; clo: the low corner of the coarse box):
//   phi_f = phi_f + phi_c(ii / 2, jj / 2, kk / 2)
template <class C>
__global__ void __launch_bounds__(MG_WG) k_mg_prolong(DFab PC, int clo0, int clo1, int clo2, DFab PF, C f)
{
    const MgLevel& L = f.L;
    const long q = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (q >= (long)L.n[0] * L.n[1] * L.n[2]) return;
    if (!C::covered(f.zone(q))) return;
    int ii, jj, kk;
    mg_zone(q, L, ii, jj, kk);
    const long at = mg_at(PF, L.lo[0] + ii, L.lo[1] + jj, L.lo[2] + kk);
    PF.p[at] = PF.p[at] + PC.p[mg_at(PC, clo0 + (ii >> 1), clo1 + (jj >> 1), clo2 + (kk >> 1))];
}

// b = fourpiG * rho on the zones of level 0: of the box of L, or (the union) gathered from the boxes' own state FABs on the
// zones of every box of the table
__global__ void __launch_bounds__(MG_WG) k_mg_rhs(DFab U, int comp, DFab B, MgLevel L, double fourpiG)
{
    const long q = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (q >= (long)L.n[0] * L.n[1] * L.n[2]) return;
    const int i = L.lo[0] + (int)(q % L.n[0]);
    const long rr = q / L.n[0];
    const int j = L.lo[1] + (int)(rr % L.n[1]), k = L.lo[2] + (int)(rr / L.n[1]);
    B.p[mg_at(B, i, j, k)] = fourpiG * U.p[mg_at(U, i, j, k) + U.sn * comp];
}

// the box of the table that holds thread t, and the zone of it
__device__ __forceinline__ bool mgb_box_zone(const MgBoxDev* __restrict__ tab, int nbox, long t, int& b, int& i, int& j, int& k)
{
    int b0 = 0, b1 = nbox - 1;
    while (b0 < b1) {
        const int mid = (b0 + b1 + 1) >> 1;
        if (tab[mid].start <= t) b0 = mid; else b1 = mid - 1;
    }
    const long r = t - tab[b0].start;
    const int n0 = tab[b0].n[0], n1 = tab[b0].n[1], n2 = tab[b0].n[2];
    if (r >= (long)n0 * n1 * n2) return false;
    const long rr = r / n0;
    b = b0;
    i = tab[b0].lo[0] + (int)(r % n0); j = tab[b0].lo[1] + (int)(rr % n1); k = tab[b0].lo[2] + (int)(rr / n1);
    return true;
}

__global__ void __launch_bounds__(MG_WG) k_mgb_rhs(const MgBoxDev* __restrict__ tab, int nbox, long total, int comp, DFab B, double fourpiG)
{
    const long t = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (t >= total) return;
    int b, i, j, k;
    if (!mgb_box_zone(tab, nbox, t, b, i, j, k)) return;
    const DFab U = tab[b].F;
    B.p[mg_at(B, i, j, k)] = fourpiG * U.p[mg_at(U, i, j, k) + U.sn * comp];
}

// a maximum that keeps a NaN once it has seen one
__device__ __forceinline__ double mg_max(double m, double v) { return (v > m || v != v) ? v : m; }

// the maxima of a workgroup of WG threads: across each wave, through the LDS, across the waves; threads 0 and 1 write them
template <int WG>
__device__ __forceinline__ void mg_max_workgroup(double ma, double mx, double* out)
{
    for (int off = 32; off > 0; off >>= 1) {
        ma = mg_max(ma, __shfl_down(ma, off, 64));
        mx = mg_max(mx, __shfl_down(mx, off, 64));
    }
    __shared__ double sa[WG / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sa[wave][0] = ma; sa[wave][1] = mx; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double m = sa[0][threadIdx.x];
        for (int w = 1; w < WG / 64; ++w) m = mg_max(m, sa[w][threadIdx.x]);
        out[threadIdx.x] = m;
    }
}

// The norm.  out[0] = max |x|, out[1] = max x over the zones of the level; a NaN anywhere gives NaN.  A maximum does not depend
// on the order it is taken in
template <class C>
__global__ void __launch_bounds__(MG_WG) k_mg_norm_partial(DFab X, C c, double* __restrict__ ws)
{
    const MgLevel& L = c.L;
    const long total = (long)L.n[0] * L.n[1] * L.n[2];
    double ma = 0.0, mx = -HUGE_VAL;
    for (long q = (long)blockIdx.x * MG_WG + threadIdx.x; q < total; q += (long)gridDim.x * MG_WG) {
        if (!C::covered(c.zone(q))) continue;
        const int i = L.lo[0] + (int)(q % L.n[0]);
        const long rr = q / L.n[0];
        const int j = L.lo[1] + (int)(rr % L.n[1]), k = L.lo[2] + (int)(rr / L.n[1]);
        const double v = X.p[mg_at(X, i, j, k)];
        ma = mg_max(ma, fabs(v));
        mx = mg_max(mx, v);
    }
    mg_max_workgroup<MG_WG>(ma, mx, ws + 2 * (long)blockIdx.x);
}

__global__ void __launch_bounds__(MG_NORM_MAX_WG) k_mg_norm_final(const double* __restrict__ ws, int nrows, double* __restrict__ out)
{
    double ma = 0.0, mx = -HUGE_VAL;
    if ((int)threadIdx.x < nrows) { ma = ws[2 * threadIdx.x]; mx = ws[2 * threadIdx.x + 1]; }
    mg_max_workgroup<MG_NORM_MAX_WG>(ma, mx, out);
}

// Gravity from phi on the zone (i, j, k) of level 0: face gradients
//   gl = (p - xm) / hx, gh = (xp - p) / hx, across an edge of the level gl = (2.0 * (p - f)) / hx, gh = (2.0 * (f - p)) / hx (the
//   linear ghost; f the value ON the face: one ghost zone of phi holds it, or the face array); a neighbour in a sibling box of a
//   union is an ordinary neighbour;
//   g_x = -(0.5 * (gl + gh)), and the same in y and z
template <class E>
__device__ __forceinline__ void mg_grad_zone(const DFab& P, const DFab& G, const E& e, int i, int j, int k, double hx, double hy, double hz)
{
    const int rel[3] = { i - e.L.lo[0], j - e.L.lo[1], k - e.L.lo[2] };
    const unsigned fl = e.zone(mg_flag_at(e.L, rel[0], rel[1], rel[2]));
    const double* p = P.p + mg_at(P, i, j, k);
    const double pc = p[0];
    const double lo[3] = { p[-1], p[-P.sy], p[-P.sz] }, hi[3] = { p[1], p[P.sy], p[P.sz] };
    const double h[3] = { hx, hy, hz };
    const long g = mg_at(G, i, j, k);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double dl = pc - lo[d], dh = hi[d] - pc;
        if (e.edge(fl, rel, d, 0)) dl = 2.0 * (pc - e.on_edge(d, 0, i, j, k, lo[d]));
        if (e.edge(fl, rel, d, 1)) dh = 2.0 * (e.on_edge(d, 1, i, j, k, hi[d]) - pc);
        const double gl = dl / h[d], gh = dh / h[d];
        G.p[g + G.sn * d] = -(0.5 * (gl + gh));
    }
}

// on the zones of the box of L, and on the zones of every box of the table, into that box's own FAB
__global__ void __launch_bounds__(MG_WG) k_grad_phi(DFab P, DFab G, MgLevel L, double hx, double hy, double hz)
{
    const long q = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (q >= (long)L.n[0] * L.n[1] * L.n[2]) return;
    int ii, jj, kk;
    mg_zone(q, L, ii, jj, kk);
    mg_grad_zone(P, G, MgOneBox{ { L } }, L.lo[0] + ii, L.lo[1] + jj, L.lo[2] + kk, hx, hy, hz);
}

__global__ void __launch_bounds__(MG_WG) k_mgb_grad(const MgBoxDev* __restrict__ tab, int nbox, long total, DFab P, MgBoxes e,
                                                   double hx, double hy, double hz)
{
    const long t = (long)blockIdx.x * MG_WG + threadIdx.x;
    if (t >= total) return;
    int b, i, j, k;
    if (!mgb_box_zone(tab, nbox, t, b, i, j, k)) return;
    mg_grad_zone(P, tab[b].F, e, i, j, k, hx, hy, hz);
}

// ---- the plan and the V-cycle -------------------------------------------------------------------------------------------------
static unsigned mg_blocks(long n) { return (unsigned)((n + MG_WG - 1) / MG_WG); }
static long mg_zones(const MgLevel& L) { return (long)L.n[0] * L.n[1] * L.n[2]; }
static long mg_pairs(const MgLevel& L) { return (long)((L.n[0] + 1) >> 1) * L.n[1] * L.n[2]; }

// The levels below the box L (n and lo set) of zones dx: coarsened while the extents are even with n / 2 >= 2, there are fewer
// than MG_MAX_LEVELS levels and -- a union of nbox boxes (lo, hi: 3 ints per box; nbox = 0: L is the level) -- every box's lo
// and hi + 1 are divisible by 2^(m+1): the 8 children of a coarse zone are then all covered or all not
static int mg_coarsen(MgLevel L, const double dx[3], int nbox, const int* lo, const int* hi, std::vector<MgLevel>& lev)
{
    double h[3] = { dx[0], dx[1], dx[2] };
    for (;;) {
        L.cx = 1.0 / (h[0] * h[0]); L.cy = 1.0 / (h[1] * h[1]); L.cz = 1.0 / (h[2] * h[2]);
        L.cdiag = 2.0 * ((L.cx + L.cy) + L.cz);
        lev.push_back(L);
        bool more = (int)lev.size() < MG_MAX_LEVELS;
        for (int d = 0; d < 3; ++d) more = more && L.n[d] % 2 == 0 && L.n[d] / 2 >= 2;
        const int m1 = (1 << (int)lev.size()) - 1;
        for (int q = 0; q < 3 * nbox && more; ++q) more = (lo[q] & m1) == 0 && ((hi[q] + 1) & m1) == 0;
        if (!more) break;
        for (int d = 0; d < 3; ++d) { L.n[d] /= 2; L.lo[d] = L.lo[d] >> 1; h[d] = 2.0 * h[d]; }
    }
    if (mg_zones(lev.back()) > CASTRO_AMD_POISSON_MAX_BOTTOM) return CASTRO_AMD_ERR_UNSUPPORTED;
    return 0;
}

int poisson_levels(const int n[3], const int lo[3], const double dx[3], std::vector<MgLevel>& lev)
{
    lev.clear();
    MgLevel L;
    std::memset(&L, 0, sizeof(L));
    for (int d = 0; d < 3; ++d) {
        if (n[d] < 1 || !(dx[d] > 0.0)) return CASTRO_AMD_ERR_ARG;
        L.n[d] = n[d]; L.lo[d] = lo[d];
    }
    return mg_coarsen(L, dx, 0, nullptr, nullptr, lev);
}

void poisson_plan_free(PoissonPlan* P)
{
    if (!P) return;
    for (double* q : P->owned) if (q) (void)hipFree(q);
    for (unsigned char* q : P->flags) if (q) (void)hipFree(q);
    P->tables.release();
    if (P->h_norm) (void)hipHostFree(P->h_norm);
    delete P;
}

// a plan-owned array of level L with `ng` ghost zones, zeroed
static int plan_array(PoissonPlan* P, const MgLevel& L, int ng, DFab& F)
{
    const long nx = L.n[0] + 2 * ng, ny = L.n[1] + 2 * ng, nz = L.n[2] + 2 * ng;
    double* q = nullptr;
    if (hipMalloc(&q, (size_t)(nx * ny * nz) * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
    P->owned.push_back(q);
    if (hipMemset(q, 0, (size_t)(nx * ny * nz) * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_HIP;
    F.p = q;
    for (int d = 0; d < 3; ++d) F.lo[d] = L.lo[d] - ng;
    F.sy = nx; F.sz = nx * ny; F.sn = nx * ny * nz;
    return 0;
}

int poisson_plan_make(const int n[3], const int lo[3], const double dx[3], PoissonPlan** out)
{
    std::vector<MgLevel> lev;
    const int rl = poisson_levels(n, lo, dx, lev);
    if (rl != 0) return rl;
    PoissonPlan* P = new (std::nothrow) PoissonPlan();
    if (!P) return CASTRO_AMD_ERR_NOMEM;
    P->lev = lev;
    const size_t nl = lev.size();
    P->phi.resize(nl); P->rhs.resize(nl); P->res.resize(nl);
    for (int d = 0; d < 3; ++d) P->dx[d] = dx[d];
    int rc = 0;
    for (size_t l = 0; l < nl && rc == 0; ++l) {
        // the ghost zones of a coarser level's correction stay zero for the life of the plan: no kernel writes them
        if (l > 0) rc = plan_array(P, lev[l], 1, P->phi[l]);
        if (rc == 0) rc = plan_array(P, lev[l], 0, P->rhs[l]);
        if (rc == 0 && l + 1 < nl) rc = plan_array(P, lev[l], 0, P->res[l]);
    }
    if (rc == 0 && nl == 1) rc = plan_array(P, lev[0], 0, P->res[0]);
    double* q = nullptr;
    if (rc == 0 && hipMalloc(&q, (4 + 2 * MG_NORM_MAX_WG) * sizeof(double)) != hipSuccess) rc = CASTRO_AMD_ERR_NOMEM;
    if (rc == 0) { P->owned.push_back(q); P->d_norm = q; P->norm_ws = q + 4; }
    if (rc == 0 && hipHostMalloc(&P->h_norm, 4 * sizeof(double)) != hipSuccess) rc = CASTRO_AMD_ERR_NOMEM;
    if (rc != 0) { poisson_plan_free(P); return rc; }
    *out = P;
    return 0;
}

// one launch under its profiler name
template <class... KA, class... A>
static int mg_launch(Profiler* prof, const char* name, void (*kernel)(KA...), unsigned nblocks, int wg, hipStream_t s, const A&... a)
{
    prof_begin(prof, name, s);
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(wg), 0, s, a...);
    prof_end(prof, s);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// The launchers pick the instantiation of a pass from the edge of the level (MgEdge, ctu_kernels.h): flags == nullptr is one box
int launch_mg_smooth(const DFab& P, const DFab& B, const MgLevel& L, const MgEdge& e, int colour, hipStream_t s, Profiler* prof)
{
    const unsigned nb = mg_blocks(mg_pairs(L));
    return e.flags ? mg_launch(prof, "k_mgb_smooth", k_mg_smooth<MgBoxes>, nb, MG_WG, s, P, B, MgBoxes{ { L, e.flags }, e.X }, colour)
                   : mg_launch(prof, "k_mg_smooth", k_mg_smooth<MgOneBox>, nb, MG_WG, s, P, B, MgOneBox{ { L } }, colour);
}

static int mg_bottom(const DFab& P, const DFab& B, const MgLevel& L, const MgEdge& e, hipStream_t s, Profiler* prof)
{
    return e.flags ? mg_launch(prof, "k_mgb_bottom", k_mg_bottom<MgBoxes>, 1, MG_BOTTOM_WG, s, P, B, MgBoxes{ { L, e.flags }, e.X }, MG_NBOTTOM)
                   : mg_launch(prof, "k_mg_bottom", k_mg_bottom<MgOneBox>, 1, MG_BOTTOM_WG, s, P, B, MgOneBox{ { L } }, MG_NBOTTOM);
}

int launch_mg_residual(const DFab& P, const DFab& B, const DFab& R, const MgLevel& L, const MgEdge& e, hipStream_t s, Profiler* prof)
{
    const unsigned nb = mg_blocks(mg_zones(L));
    return e.flags ? mg_launch(prof, "k_mgb_residual", k_mg_residual<MgBoxes>, nb, MG_WG, s, P, B, R, MgBoxes{ { L, e.flags }, e.X })
                   : mg_launch(prof, "k_mg_residual", k_mg_residual<MgOneBox>, nb, MG_WG, s, P, B, R, MgOneBox{ { L } });
}

// cflags, fflags, flags: the coverage of the coarse / the fine / the level, nullptr for one box
int launch_mg_restrict(const DFab& RF, const MgLevel& LF, const DFab& BC, const DFab& PC, const MgLevel& LC, const unsigned char* cflags,
                       hipStream_t s, Profiler* prof)
{
    const unsigned nb = mg_blocks(mg_zones(LC));
    return cflags ? mg_launch(prof, "k_mgb_restrict", k_mg_restrict<MgMasked>, nb, MG_WG, s, RF, LF.lo[0], LF.lo[1], LF.lo[2], BC, PC, MgMasked{ LC, cflags })
                  : mg_launch(prof, "k_mg_restrict", k_mg_restrict<MgWhole>, nb, MG_WG, s, RF, LF.lo[0], LF.lo[1], LF.lo[2], BC, PC, MgWhole{ LC });
}

int launch_mg_prolong(const DFab& PC, const MgLevel& LC, const DFab& PF, const MgLevel& LF, const unsigned char* fflags, hipStream_t s,
                      Profiler* prof)
{
    const unsigned nb = mg_blocks(mg_zones(LF));
    return fflags ? mg_launch(prof, "k_mgb_prolong", k_mg_prolong<MgMasked>, nb, MG_WG, s, PC, LC.lo[0], LC.lo[1], LC.lo[2], PF, MgMasked{ LF, fflags })
                  : mg_launch(prof, "k_mg_prolong", k_mg_prolong<MgWhole>, nb, MG_WG, s, PC, LC.lo[0], LC.lo[1], LC.lo[2], PF, MgWhole{ LF });
}

int launch_mg_norm(const DFab& X, const MgLevel& L, const unsigned char* flags, double* ws, double* d_out, hipStream_t s, Profiler* prof)
{
    unsigned nb = mg_blocks(mg_zones(L));
    if (nb > (unsigned)MG_NORM_MAX_WG) nb = MG_NORM_MAX_WG;
    const int rc = flags ? mg_launch(prof, "k_mgb_norm_partial", k_mg_norm_partial<MgMasked>, nb, MG_WG, s, X, MgMasked{ L, flags }, ws)
                         : mg_launch(prof, "k_mg_norm_partial", k_mg_norm_partial<MgWhole>, nb, MG_WG, s, X, MgWhole{ L }, ws);
    return rc != 0 ? rc : mg_launch(prof, "k_mg_norm_final", k_mg_norm_final, 1, MG_NORM_MAX_WG, s, ws, (int)nb, d_out);
}

// the edge of level l of the plan; X: the face values of level 0 of a union (the coarser levels have none: 0.0; X.p == nullptr for
// one box, whose ghost zones of phi hold them)
static MgEdge mg_edge(const PoissonPlan* P, size_t l, const DFab& X)
{
    MgEdge e;
    std::memset(&e, 0, sizeof(e));
    if (!P->flags.empty()) e.flags = P->flags[l];
    if (l == 0) e.X = X;
    return e;
}

// One V-cycle from level l down: MG_NPRE sweeps (colour 0, colour 1), residual, restriction, the coarser levels, prolongation,
// MG_NPOST sweeps; the coarsest level is the bottom solve alone
static int mg_vcycle(PoissonPlan* P, size_t l, const DFab& X, hipStream_t s, Profiler* prof)
{
    const MgLevel& L = P->lev[l];
    const MgEdge e = mg_edge(P, l, X);
    int rc = 0;
    if (l + 1 == P->lev.size()) return mg_bottom(P->phi[l], P->rhs[l], L, e, s, prof);
    const unsigned char* cflags = mg_edge(P, l + 1, X).flags;
    for (int it = 0; it < MG_NPRE && rc == 0; ++it)
        for (int colour = 0; colour < 2 && rc == 0; ++colour) rc = launch_mg_smooth(P->phi[l], P->rhs[l], L, e, colour, s, prof);
    if (rc == 0) rc = launch_mg_residual(P->phi[l], P->rhs[l], P->res[l], L, e, s, prof);
    if (rc == 0) rc = launch_mg_restrict(P->res[l], L, P->rhs[l + 1], P->phi[l + 1], P->lev[l + 1], cflags, s, prof);
    if (rc == 0) rc = mg_vcycle(P, l + 1, X, s, prof);
    if (rc == 0) rc = launch_mg_prolong(P->phi[l + 1], P->lev[l + 1], P->phi[l], L, e.flags, s, prof);
    for (int it = 0; it < MG_NPOST && rc == 0; ++it)
        for (int colour = 0; colour < 2 && rc == 0; ++colour) rc = launch_mg_smooth(P->phi[l], P->rhs[l], L, e, colour, s, prof);
    return rc;
}

// the residual of level 0 into the scratch of the plan (res[0]; the V-cycle overwrites it again), its norm into d_norm[at..at+1]
static int mg_residual_norm(PoissonPlan* P, const DFab& X, int at, hipStream_t s, Profiler* prof)
{
    const MgEdge e = mg_edge(P, 0, X);
    int rc = launch_mg_residual(P->phi[0], P->rhs[0], P->res[0], P->lev[0], e, s, prof);
    if (rc == 0) rc = launch_mg_norm(P->res[0], P->lev[0], e.flags, P->norm_ws, P->d_norm + at, s, prof);
    return rc;
}

static int mg_read(PoissonPlan* P, int n, hipStream_t s)
{
    if (hipMemcpyAsync(P->h_norm, P->d_norm, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) return CASTRO_AMD_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// V-cycles on phi[0] with the right-hand side rhs[0] of the plan until the residual norm is below the tolerance or maxiter is spent
static int mg_solve(PoissonPlan* P, const DFab& X, double reltol, double abstol, int maxiter, int* cycles, int* converged,
                    double* final_norm, double* h_history, hipStream_t s, Profiler* prof)
{
    int rc = launch_mg_norm(P->rhs[0], P->lev[0], mg_edge(P, 0, X).flags, P->norm_ws, P->d_norm, s, prof);
    if (rc == 0) rc = mg_residual_norm(P, X, 2, s, prof);
    if (rc == 0) rc = mg_read(P, 4, s);
    if (rc != 0) return rc;
    const double bnorm = P->h_norm[0], max_rhs = P->h_norm[1];
    double rnorm = P->h_norm[2];
    const double t1 = reltol * bnorm, t2 = abstol * max_rhs;
    const double tol = t1 > t2 ? t1 : t2;
    if (h_history) { h_history[0] = bnorm; h_history[1] = max_rhs; h_history[2] = rnorm; }
    int n = 0;
    while (!(rnorm <= tol) && n < maxiter) {
        rc = mg_vcycle(P, 0, X, s, prof);
        if (rc == 0) rc = mg_residual_norm(P, X, 0, s, prof);
        if (rc == 0) rc = mg_read(P, 1, s);
        if (rc != 0) return rc;
        rnorm = P->h_norm[0];
        ++n;
        if (h_history) h_history[2 + n] = rnorm;
    }
    *cycles = n;
    *converged = rnorm <= tol ? 1 : 0;
    *final_norm = rnorm;
    return 0;
}

int launch_poisson_solve(PoissonPlan* P, const DFab& phi, const DFab& U, int comp, double fourpiG, double reltol, double abstol,
                         int maxiter, int* cycles, int* converged, double* final_norm, double* h_history, hipStream_t s, Profiler* prof)
{
    P->phi[0] = phi;
    const MgLevel& L0 = P->lev[0];
    const int rc = mg_launch(prof, "k_mg_rhs", k_mg_rhs, mg_blocks(mg_zones(L0)), MG_WG, s, U, comp, P->rhs[0], L0, fourpiG);
    if (rc != 0) return rc;
    DFab none;
    std::memset(&none, 0, sizeof(none));
    return mg_solve(P, none, reltol, abstol, maxiter, cycles, converged, final_norm, h_history, s, prof);
}

int launch_grad_phi(const DFab& phi, const DFab& G, const MgLevel& L, const double dx[3], hipStream_t s, Profiler* prof)
{
    return mg_launch(prof, "k_grad_phi", k_grad_phi, mg_blocks(mg_zones(L)), MG_WG, s, phi, G, L, dx[0], dx[1], dx[2]);
}

// ---- the plan of a level that is a union of boxes: ONE array over the bounding box, a byte of flags per zone ------------------------
// The levels of a union of boxes (lo, hi: 3 ints per box, in the zones of level 0): level m is the bounding box >> m, coarsened
// by mg_coarsen's rule with the alignment of the boxes
int poisson_boxes_levels(int nbox, const int* lo, const int* hi, const double dx[3], std::vector<MgLevel>& lev)
{
    lev.clear();
    if (nbox < 1 || !lo || !hi) return CASTRO_AMD_ERR_ARG;
    MgLevel L;
    std::memset(&L, 0, sizeof(L));
    int bhi[3];
    for (int d = 0; d < 3; ++d) {
        if (!(dx[d] > 0.0)) return CASTRO_AMD_ERR_ARG;
        L.lo[d] = lo[d]; bhi[d] = hi[d];
    }
    for (int b = 0; b < nbox; ++b)
        for (int d = 0; d < 3; ++d) {
            const int l = lo[3 * b + d], u = hi[3 * b + d];
            // the refinement of a coarse box inside a non-negative index space
            if (u < l || l < 0 || u > (1 << 30) || (l & 1) != 0 || (u & 1) != 1) return CASTRO_AMD_ERR_ARG;
            if (l < L.lo[d]) L.lo[d] = l;
            if (u > bhi[d]) bhi[d] = u;
        }
    for (int b = 0; b < nbox; ++b)
        for (int c = 0; c < b; ++c) {
            bool apart = false;
            for (int d = 0; d < 3; ++d) apart = apart || hi[3 * b + d] < lo[3 * c + d] || hi[3 * c + d] < lo[3 * b + d];
            if (!apart) return CASTRO_AMD_ERR_ARG;
        }
    for (int d = 0; d < 3; ++d) L.n[d] = bhi[d] - L.lo[d] + 1;
    return mg_coarsen(L, dx, nbox, lo, hi, lev);
}

// the flags of level m (shift = m) of the union
static void mgb_flags(int nbox, const int* lo, const int* hi, const MgLevel& L, int shift, std::vector<unsigned char>& f)
{
    const long n0 = L.n[0], n1 = L.n[1], n2 = L.n[2];
    f.assign((size_t)(n0 * n1 * n2), 0);
    for (int b = 0; b < nbox; ++b) {
        int l[3], u[3];
        for (int d = 0; d < 3; ++d) { l[d] = (lo[3 * b + d] >> shift) - L.lo[d]; u[d] = (hi[3 * b + d] >> shift) - L.lo[d]; }
        for (int k = l[2]; k <= u[2]; ++k)
            for (int j = l[1]; j <= u[1]; ++j)
                for (int i = l[0]; i <= u[0]; ++i) f[(size_t)(i + n0 * (j + n1 * k))] = MGF_COVERED;
    }
    const long st[3] = { 1, n0, n0 * n1 };
    for (long k = 0; k < n2; ++k)
        for (long j = 0; j < n1; ++j)
            for (long i = 0; i < n0; ++i) {
                const long q = i + n0 * (j + n1 * k);
                if (!(f[(size_t)q] & MGF_COVERED)) continue;
                const long at[3] = { i, j, k }, n[3] = { n0, n1, n2 };
                unsigned v = f[(size_t)q];
                for (int d = 0; d < 3; ++d) {
                    if (at[d] == 0 || !(f[(size_t)(q - st[d])] & MGF_COVERED)) v |= mgf_face(d, 0);
                    if (at[d] == n[d] - 1 || !(f[(size_t)(q + st[d])] & MGF_COVERED)) v |= mgf_face(d, 1);
                }
                f[(size_t)q] = (unsigned char)v;
            }
}

int poisson_boxes_plan_make(int nbox, const int* lo, const int* hi, const double dx[3], PoissonPlan** out)
{
    std::vector<MgLevel> lev;
    const int rl = poisson_boxes_levels(nbox, lo, hi, dx, lev);
    if (rl != 0) return rl;
    PoissonPlan* P = nullptr;
    const int rp = poisson_plan_make(lev[0].n, lev[0].lo, dx, &P);
    if (rp != 0) return rp;
    // the alignment of the boxes may stop the coarsening before the extents do: the levels below are not used
    P->lev.resize(lev.size());
    P->boxes.resize((size_t)(6 * nbox));
    for (int b = 0; b < nbox; ++b)
        for (int d = 0; d < 3; ++d) { P->boxes[(size_t)(6 * b + d)] = lo[3 * b + d]; P->boxes[(size_t)(6 * b + 3 + d)] = hi[3 * b + d]; }
    std::vector<unsigned char> f;
    for (size_t m = 0; m < lev.size(); ++m) {
        mgb_flags(nbox, lo, hi, lev[m], (int)m, f);
        unsigned char* q = nullptr;
        if (hipMalloc(&q, f.size()) != hipSuccess) { poisson_plan_free(P); return CASTRO_AMD_ERR_NOMEM; }
        P->flags.push_back(q);
        if (hipMemcpy(q, f.data(), f.size(), hipMemcpyHostToDevice) != hipSuccess) { poisson_plan_free(P); return CASTRO_AMD_ERR_HIP; }
    }
    *out = P;
    return 0;
}

// the table of the boxes of the plan with the FABs F, on the device (a table the plan has seen costs no copy)
static int mgb_table(PoissonPlan* P, const DFab* F, hipStream_t s, const MgBoxDev*& dtab, long& total)
{
    const size_t nbox = P->boxes.size() / 6;
    std::vector<MgBoxDev> tab(nbox);
    std::memset((void*)tab.data(), 0, nbox * sizeof(MgBoxDev));
    total = 0;
    for (size_t b = 0; b < nbox; ++b) {
        tab[b].F = F[b];
        long n = 1;
        for (int d = 0; d < 3; ++d) {
            tab[b].lo[d] = P->boxes[6 * b + d];
            tab[b].n[d] = P->boxes[6 * b + 3 + d] - P->boxes[6 * b + d] + 1;
            n *= tab[b].n[d];
        }
        tab[b].start = total;
        total += n;
    }
    return P->tables.find(tab.data(), nbox, s, dtab);
}

int launch_poisson_boxes_solve(PoissonPlan* P, const DFab& phi, const DFab& X, const DFab* U, int comp, double fourpiG, double reltol,
                               double abstol, int maxiter, int* cycles, int* converged, double* final_norm, double* h_history,
                               hipStream_t s, Profiler* prof)
{
    P->phi[0] = phi;
    const MgBoxDev* dtab;
    long total;
    int rc = mgb_table(P, U, s, dtab, total);
    if (rc != 0) return rc;
    rc = mg_launch(prof, "k_mgb_rhs", k_mgb_rhs, mg_blocks(total), MG_WG, s, dtab, (int)(P->boxes.size() / 6), total, comp, P->rhs[0], fourpiG);
    if (rc != 0) return rc;
    return mg_solve(P, X, reltol, abstol, maxiter, cycles, converged, final_norm, h_history, s, prof);
}

int launch_grad_phi_boxes(PoissonPlan* P, const DFab& phi, const DFab& X, const DFab* G, hipStream_t s, Profiler* prof)
{
    const MgBoxDev* dtab;
    long total;
    const int rc = mgb_table(P, G, s, dtab, total);
    if (rc != 0) return rc;
    return mg_launch(prof, "k_mgb_grad", k_mgb_grad, mg_blocks(total), MG_WG, s, dtab, (int)(P->boxes.size() / 6), total, phi,
                     MgBoxes{ { P->lev[0], P->flags[0] }, X }, P->dx[0], P->dx[1], P->dx[2]);
}

} // namespace cad

// ---- multipole moments and the boundary potential: no contraction in either build --------------------------------------------
#pragma clang fp contract(off)

namespace cad {

constexpr int MP_MAX = CASTRO_AMD_MAX_MULTIPOLE;
constexpr int MP_NC = 2 * (MP_MAX + 1);          // accumulators of a thread: cosine and sine parts of l = 0 .. MP_MAX
constexpr int MP_WG = 256;
constexpr int MP_MAX_WG = 1024;                  // workgroups per m: a thread takes more zones rather than the grid growing beyond it
constexpr int MP_FINAL_GROUPS = 16;
constexpr int MP_FINAL_WG = 576;                 // MP_FINAL_GROUPS * MP_NC = 544 threads at work, rounded up to whole waves
static_assert(MP_FINAL_GROUPS * MP_NC <= MP_FINAL_WG && MP_FINAL_WG % 64 == 0, "k_mp_final's thread layout");

// factorial of Gravity_util.H
__host__ __device__ inline double mp_factorial(int n)
{
    double fact = 1.0;
    for (int i = 2; i <= n; ++i) fact *= (double)i;
    return fact;
}

// calcLegPolyL of Gravity_util.H
__device__ __forceinline__ void mp_leg(int l, double& p, double& p1, double& p2, double x)
{
    if (l == 0) p = 1.0;
    else if (l == 1) { p1 = p; p = x; }
    else { p2 = p1; p1 = p; p = ((2 * l - 1) * x * p1 - (l - 1) * p2) / l; }
}

// calcAssocLegPolyLM of Gravity_util.H
__device__ __forceinline__ void mp_assoc(int l, int m, double& a, double& a1, double& a2, double x)
{
    if (l == m) {
        a = ((m & 1) ? -1.0 : 1.0) * pow((1.0 - x) * (1.0 + x), m * 0.5);        // std::pow(-1, m) is exactly -1 or 1
        for (int n = 2 * m - 1; n >= 3; n = n - 2) a *= n;
    } else if (l == m + 1) {
        a1 = a;
        a = x * (2 * m + 1) * a1;
    } else {
        a2 = a1; a1 = a;
        a = (x * (2 * l - 1) * a1 - (l + m - 1) * a2) / (l - m);
    }
}

// The moments of order m = blockIdx.y.  A workgroup takes the zones base + it * MP_WG + thread, it = 0 .. iters - 1, of one box (x
// fastest); a thread adds the terms of its zones in that order -- for m = 0 dQL0(l) = ((legPolyL * (rho * pow(r, l))) * vol), for
// m > 0 dQLC(l, m) = ((((assoc * cos(m * phiAngle)) * (rho * pow(r, l))) * vol) * factArray(l, m)) and the same with sin,
// l = m .. lnum (multipole_add, volumeFactor = 1 and the parity factors 1: no Symmetry face) --, the 64 lanes of a wave are added
// pairwise (32, 16, ... 1), the four waves in wave order, and the workgroup stores ONE row of MP_NC doubles.
__global__ void __launch_bounds__(MP_WG) k_mp_partial(const DiagBoxDev* __restrict__ tab, const int* __restrict__ start, int nbox,
                                                     int iters, MpGeom G, double* __restrict__ ws)
{
    const int m = blockIdx.y, lnum = G.lnum;
    __shared__ double sfact[MP_MAX + 1];
    if ((int)threadIdx.x <= MP_MAX) {
        const int l = threadIdx.x;
        sfact[l] = (m >= 1 && l >= m && l <= lnum) ? 2.0 * mp_factorial(l - m) / mp_factorial(l + m) : 0.0;
    }
    __syncthreads();
    const unsigned bid = blockIdx.x;
    int b0 = 0, b1 = nbox - 1;
    while (b0 < b1) {
        const int mid = (b0 + b1 + 1) >> 1;
        if ((unsigned)start[mid] <= bid) b0 = mid; else b1 = mid - 1;
    }
    const DiagBoxDev B = tab[b0];
    const long total = (long)B.n[0] * B.n[1] * B.n[2];
    const long base = (long)(bid - (unsigned)start[b0]) * MP_WG * iters + threadIdx.x;

    double ac[MP_MAX + 1], as[MP_MAX + 1];
#pragma unroll
    for (int l = 0; l <= MP_MAX; ++l) { ac[l] = 0.0; as[l] = 0.0; }

    const double rmax_cubed_inv = 1.0 / (G.rmax * G.rmax * G.rmax);
    const double vol = (G.dx[0] * G.dx[1] * G.dx[2]) * rmax_cubed_inv;
    for (int it = 0; it < iters; ++it) {
        const long q = base + (long)it * MP_WG;
        if (q >= total) break;
        const int ii = (int)(q % B.n[0]);
        const long rr = q / B.n[0];
        const int jj = (int)(rr % B.n[1]), kk = (int)(rr / B.n[1]);
        if (B.mask && B.mask[q] == 0) continue;
        const int i = B.lo[0] + ii, j = B.lo[1] + jj, k = B.lo[2] + kk;
        const double rho = B.U.p[(long)(i - B.U.lo[0]) + B.U.sy * (long)(j - B.U.lo[1]) + B.U.sz * (long)(k - B.U.lo[2]) + B.U.sn * URHO];
        const double x = (G.problo[0] + ((double)i + 0.5) * G.dx[0] - G.center[0]) / G.rmax;
        const double y = (G.problo[1] + ((double)j + 0.5) * G.dx[1] - G.center[1]) / G.rmax;
        const double z = (G.problo[2] + ((double)k + 0.5) * G.dx[2] - G.center[2]) / G.rmax;
        const double r = sqrt(x * x + y * y + z * z);
        const double cosTheta = z / r;
        // the loop over l is not unrolled (one copy of pow); the accumulator of l -- a register -- is picked by a uniform test
        double cm = 0.0, sm = 0.0;
        if (m > 0) {
            const double phiAngle = atan2(y, x);
            cm = cos(m * phiAngle);
            sm = sin(m * phiAngle);
        }
        double a = 0.0, a1 = 0.0, a2 = 0.0;
#pragma nounroll
        for (int l = m; l <= lnum; ++l) {
            const double rho_r_L = rho * pow(r, (double)l);
            double tc, ts = 0.0;
            if (m == 0) {
                mp_leg(l, a, a1, a2, cosTheta);
                tc = a * rho_r_L * vol;
            } else {
                mp_assoc(l, m, a, a1, a2, cosTheta);
                tc = a * cm * rho_r_L * vol * sfact[l];
                ts = a * sm * rho_r_L * vol * sfact[l];
            }
#pragma unroll
            for (int ll = 0; ll <= MP_MAX; ++ll)
                if (ll == l) { ac[ll] += tc; as[ll] += ts; }
        }
    }

    __shared__ double sa[MP_WG / 64][MP_NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int l = 0; l <= MP_MAX; ++l) {
        double c = ac[l], s = as[l];
        for (int off = 32; off > 0; off >>= 1) { c += __shfl_down(c, off, 64); s += __shfl_down(s, off, 64); }
        if (lane == 0) { sa[wave][2 * l] = c; sa[wave][2 * l + 1] = s; }
    }
    __syncthreads();
    if ((int)threadIdx.x < MP_NC) {
        const int t = threadIdx.x;
        ws[((long)m * gridDim.x + bid) * MP_NC + t] = ((sa[0][t] + sa[1][t]) + sa[2][t]) + sa[3][t];
    }
}

// m = blockIdx.x: group g adds the rows g, g + 16, g + 32, ... of that m in row order, then the 16 groups are added in group
// order.  out[((kind * (lnum + 1)) + l) * (lnum + 1) + m]: kind 0 = qL0 (m = 0), 1 = qLC, 2 = qLS; the caller has zeroed `out`
__global__ void __launch_bounds__(MP_FINAL_WG) k_mp_final(const double* __restrict__ ws, int nrows, int lnum, double* __restrict__ out)
{
    __shared__ double sg[MP_FINAL_GROUPS][MP_NC];
    const int m = blockIdx.x;
    const int col = threadIdx.x % MP_NC, grp = threadIdx.x / MP_NC;
    if (grp < MP_FINAL_GROUPS) {
        double acc = 0.0;
        for (int r = grp; r < nrows; r += MP_FINAL_GROUPS) acc += ws[((long)m * nrows + r) * MP_NC + col];
        sg[grp][col] = acc;
    }
    __syncthreads();
    if (grp == 0) {
        double s = sg[0][col];
        for (int g = 1; g < MP_FINAL_GROUPS; ++g) s += sg[g][col];
        const int l = col >> 1, sine = col & 1, n1 = lnum + 1;
        if (l <= lnum && l >= m) {
            if (m == 0) { if (!sine) out[l * n1] = s; }
            else out[((1 + sine) * n1 + l) * n1 + m] = s;
        }
    }
}

// The boundary potential (Gravity.cpp:2078-2216) of the zones of the six slabs of [flo, fhi] outside the domain; a zone of the
// domain is never written.  The coordinate of a direction in which the zone lies outside sits on the domain face.
__global__ void __launch_bounds__(256) k_mp_phi_bc(DFab F, Slabs S, MpGeom G, const double* __restrict__ q)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= S.start[6]) return;
    int r = 0;
    while (tid >= S.start[r + 1]) ++r;
    const long t = tid - S.start[r];
    int ijk[3];
    ijk[0] = S.lo[r][0] + (int)(t % S.nn[r][0]);
    const long rr = t / S.nn[r][0];
    ijk[1] = S.lo[r][1] + (int)(rr % S.nn[r][1]);
    ijk[2] = S.lo[r][2] + (int)(rr / S.nn[r][1]);
    double loc[3];
    bool outside = false;
    for (int d = 0; d < 3; ++d) {
        double v;
        if (ijk[d] > G.domhi[d]) { v = G.problo[d] + ((double)ijk[d]) * G.dx[d] - G.center[d]; outside = true; }
        else if (ijk[d] < G.domlo[d]) { v = G.problo[d] + ((double)(ijk[d] + 1)) * G.dx[d] - G.center[d]; outside = true; }
        else v = G.problo[d] + ((double)ijk[d] + 0.5) * G.dx[d] - G.center[d];
        loc[d] = v / G.rmax;
    }
    if (!outside) return;
    double* dst = F.p + mg_at(F, ijk[0], ijk[1], ijk[2]);
    const double x = loc[0], y = loc[1], z = loc[2];
    const double r_ = sqrt(x * x + y * y + z * z);
    if (r_ < 1.0e-12) { *dst = 0.0; return; }
    const double rmax_cubed = G.rmax * G.rmax * G.rmax;
    const double cosTheta = z / r_;
    const double phiAngle = atan2(y, x);
    const int lnum = G.lnum, n1 = lnum + 1;
    double phi = 0.0;
    {
        double p = 0.0, p1 = 0.0, p2 = 0.0;
        for (int l = 0; l <= lnum; ++l) {
            mp_leg(l, p, p1, p2, cosTheta);
            // r^(-1) of the monopole term is one correctly rounded division, not a library call: with lnum = 0 the whole
            // boundary potential is then arithmetic a restatement reproduces bit for bit (the level solves' driver test does)
            const double r_U = l == 0 ? 1.0 / r_ : pow(r_, (double)(-l - 1));
            phi += q[l * n1] * p * r_U * rmax_cubed;
        }
    }
    for (int m = 1; m <= lnum; ++m) {
        double a = 0.0, a1 = 0.0, a2 = 0.0;
        for (int l = m; l <= lnum; ++l) {
            mp_assoc(l, m, a, a1, a2, cosTheta);
            const double r_U = pow(r_, (double)(-l - 1));
            phi += (q[(n1 + l) * n1 + m] * cos(m * phiAngle) + q[(2 * n1 + l) * n1 + m] * sin(m * phiAngle)) * a * r_U * rmax_cubed;
        }
    }
    *dst = -G.Gconst * phi / G.rmax;
}

// start[r]: first workgroup of box r; iters: zones a thread takes
static int mp_layout(int nbox, const DiagBoxDev* boxes, std::vector<int>& start, int& iters)
{
    start.assign((size_t)nbox + 1, 0);
    for (iters = 1; ; iters *= 2) {
        long tot = 0;
        for (int r = 0; r < nbox; ++r) {
            const DiagBoxDev& B = boxes[r];
            const long zones = (B.n[0] > 0 && B.n[1] > 0 && B.n[2] > 0) ? (long)B.n[0] * B.n[1] * B.n[2] : 0;
            const long per = (long)MP_WG * iters;
            tot += (zones + per - 1) / per;
            start[(size_t)r + 1] = (int)(tot < 0x3fffffffL ? tot : 0x3fffffffL);
        }
        if (tot <= MP_MAX_WG || iters >= (1 << 20)) {
            if (tot > 0xffffL) return CASTRO_AMD_ERR_ARG;
            break;
        }
    }
    return 0;
}

int launch_multipole_moments(int nbox, DiagBoxDev* boxes, const MpGeom& G, StagedTable* arena, DiagWorkspace* ws, double* d_out,
                             hipStream_t stream, Profiler* prof)
{
    if (G.lnum < 0 || !(G.rmax > 0.0)) return CASTRO_AMD_ERR_ARG;
    if (G.lnum > MP_MAX) return CASTRO_AMD_ERR_UNSUPPORTED;
    const int n1 = G.lnum + 1;
    if (hipMemsetAsync(d_out, 0, (size_t)(3 * n1 * n1) * sizeof(double), stream) != hipSuccess) return CASTRO_AMD_ERR_HIP;
    std::vector<int> start;
    int iters = 1;
    if (nbox > 0) {
        for (int r = 0; r < nbox; ++r) boxes[r].npr = 0;
        const int rc = mp_layout(nbox, boxes, start, iters);
        if (rc != 0) return rc;
    }
    const int nb = nbox > 0 ? start.back() : 0;
    if (nb == 0) return 0;
    const size_t rows = (size_t)nb * (size_t)n1;
    if (rows > ws->rows) {
        const size_t want = rows > (size_t)MP_MAX_WG * (MP_MAX + 1) ? rows : (size_t)MP_MAX_WG * (MP_MAX + 1);
        if (ws->p) { (void)hipStreamSynchronize(stream); (void)hipFree(ws->p); ws->p = nullptr; ws->rows = 0; }
        if (hipMalloc(&ws->p, want * MP_NC * sizeof(double)) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
        ws->rows = want;
    }
    const DiagBoxDev* dbox;
    const int* dstart;
    const int rt = arena->stage(boxes, (size_t)nbox, start.data(), start.size(), stream, dbox, dstart);
    if (rt != 0) return rt;
    prof_begin(prof, "k_mp_partial", stream);
    hipLaunchKernelGGL(k_mp_partial, dim3((unsigned)nb, (unsigned)n1), dim3(MP_WG), 0, stream, dbox, dstart, nbox, iters, G, ws->p);
    prof_end(prof, stream);
    if (hipGetLastError() != hipSuccess) return CASTRO_AMD_ERR_HIP;
    prof_begin(prof, "k_mp_final", stream);
    hipLaunchKernelGGL(k_mp_final, dim3((unsigned)n1), dim3(MP_FINAL_WG), 0, stream, (const double*)ws->p, nb, G.lnum, d_out);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

int launch_multipole_phi_bc(const DFab& F, const int flo[3], const int fhi[3], const MpGeom& G, const double* d_q, hipStream_t stream,
                            Profiler* prof)
{
    if (G.lnum < 0 || !(G.rmax > 0.0)) return CASTRO_AMD_ERR_ARG;
    if (G.lnum > MP_MAX) return CASTRO_AMD_ERR_UNSUPPORTED;
    // the part of the FAB inside the domain: the six slabs around it are the zones to fill
    int blo[3], bhi[3];
    for (int d = 0; d < 3; ++d) {
        blo[d] = flo[d] > G.domlo[d] ? flo[d] : G.domlo[d];
        bhi[d] = fhi[d] < G.domhi[d] ? fhi[d] : G.domhi[d];
        if (bhi[d] < blo[d]) return CASTRO_AMD_ERR_ARG;
    }
    const Slabs S = shell_slabs(flo, fhi, blo, bhi);
    const long n = S.start[6];
    if (n <= 0) return 0;
    prof_begin(prof, "k_mp_phi_bc", stream);
    hipLaunchKernelGGL(k_mp_phi_bc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, F, S, G, d_q);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// ---- the coarse-fine boundary of the potential of a refined level (level solves: gravity.no_sync = 1, no_composite = 1) ----------
// The one-zone shell of the fine box [flo, fhi] in the fine FAB F, from the coarse potentials O (old) and N (new) of the level
// below (refinement ratio 2) at the fine level's time: c = oma * O + a * N with oma = 1.0 - a formed on the host (GetCrsePhi; the
// order of k_lincomb).  A face zone gets the value ON the fine face, which is what the solver keeps in its ghost zone.  Beyond an
// x face, with the fine transverse indices (j, k), J = j >> 1, K = k >> 1, I_out = i >> 1 the coarse zone under the ghost zone and
// I_in the one across the face:
//   m(J, K) = 0.5 * (c(I_out, J, K) + c(I_in, J, K))
//   value = (m(J, K) + s_j * (0.125 * (m(J + 1, K) - m(J - 1, K)))) + s_k * (0.125 * (m(J, K + 1) - m(J, K - 1)))
// s = -1.0 for an even fine index, +1.0 for an odd one; the y faces take (i, k), the z faces (i, j), the lower direction first.
// Edge and corner zones of the shell are read by no pass of the solver: 0.  Coarse zones read: the coarsened box grown by one.
// Threads: the two z layers ((nx + 2) (ny + 2) zones each, edges and corners in them), the two y layers ((nx + 2) nz), the two x
// layers (ny nz); x runs fastest in the z and y layers.  No atomics, no LDS; nothing but the shell is written.
struct CfShell { int flo[3], fhi[3]; long start[4]; };

__device__ __forceinline__ double cf_crse(const DFab& O, const DFab& N, double oma, double a, const int c[3])
{
    return oma * O.p[mg_at(O, c[0], c[1], c[2])] + a * N.p[mg_at(N, c[0], c[1], c[2])];
}

// m of the coarse transverse position c (c[d] is ignored): the mean of the coarse zones on the two sides of the face
__device__ __forceinline__ double cf_face_mean(const DFab& O, const DFab& N, double oma, double a, int d, int c_out, int c_in, const int c[3])
{
    int p[3] = { c[0], c[1], c[2] };
    p[d] = c_out;
    const double vo = cf_crse(O, N, oma, a, p);
    p[d] = c_in;
    const double vi = cf_crse(O, N, oma, a, p);
    return 0.5 * (vo + vi);
}

// the value on the face between the fine zone g, which lies outside, and its neighbour across the (d, side) face of the fine region
__device__ __forceinline__ double cf_face_value(const DFab& O, const DFab& N, double oma, double a, int d, int side, const int g[3])
{
    const int t1 = d == 0 ? 1 : 0, t2 = d == 2 ? 1 : 2;
    const int c_out = g[d] >> 1, c_in = side ? c_out - 1 : c_out + 1;
    int c[3] = { g[0] >> 1, g[1] >> 1, g[2] >> 1 };
    const double m0 = cf_face_mean(O, N, oma, a, d, c_out, c_in, c);
    c[t1] += 1;
    const double m1p = cf_face_mean(O, N, oma, a, d, c_out, c_in, c);
    c[t1] -= 2;
    const double m1m = cf_face_mean(O, N, oma, a, d, c_out, c_in, c);
    c[t1] += 1;
    c[t2] += 1;
    const double m2p = cf_face_mean(O, N, oma, a, d, c_out, c_in, c);
    c[t2] -= 2;
    const double m2m = cf_face_mean(O, N, oma, a, d, c_out, c_in, c);
    const double s1 = (g[t1] & 1) ? 1.0 : -1.0, s2 = (g[t2] & 1) ? 1.0 : -1.0;
    return (m0 + s1 * (0.125 * (m1p - m1m))) + s2 * (0.125 * (m2p - m2m));
}

__global__ void __launch_bounds__(256) k_phi_cf_bc(DFab F, DFab O, DFab N, CfShell S, double oma, double a)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= S.start[3]) return;
    const int nxg = S.fhi[0] - S.flo[0] + 3, nyg = S.fhi[1] - S.flo[1] + 3;
    const int ny = nyg - 2, nz = S.fhi[2] - S.flo[2] + 1;
    int d, side, g[3];
    if (tid < S.start[1]) {
        const long per = (long)nxg * nyg;
        const long r = tid % per;
        d = 2; side = (int)(tid / per);
        g[0] = S.flo[0] - 1 + (int)(r % nxg);
        g[1] = S.flo[1] - 1 + (int)(r / nxg);
    } else if (tid < S.start[2]) {
        const long t = tid - S.start[1], per = (long)nxg * nz;
        const long r = t % per;
        d = 1; side = (int)(t / per);
        g[0] = S.flo[0] - 1 + (int)(r % nxg);
        g[2] = S.flo[2] + (int)(r / nxg);
    } else {
        const long t = tid - S.start[2], per = (long)ny * nz;
        const long r = t % per;
        d = 0; side = (int)(t / per);
        g[1] = S.flo[1] + (int)(r % ny);
        g[2] = S.flo[2] + (int)(r / ny);
    }
    g[d] = side ? S.fhi[d] + 1 : S.flo[d] - 1;
    double* dst = F.p + mg_at(F, g[0], g[1], g[2]);
    int nout = 0;
    for (int e = 0; e < 3; ++e) nout += (g[e] < S.flo[e] || g[e] > S.fhi[e]) ? 1 : 0;
    if (nout != 1) { *dst = 0.0; return; }
    *dst = cf_face_value(O, N, oma, a, d, side, g);
}

int launch_phi_cf_bc(const DFab& F, const int flo[3], const int fhi[3], const DFab& O, const DFab& N, double a, hipStream_t stream,
                     Profiler* prof)
{
    CfShell S;
    long n[3];
    for (int d = 0; d < 3; ++d) {
        if (fhi[d] < flo[d]) return CASTRO_AMD_ERR_ARG;
        S.flo[d] = flo[d]; S.fhi[d] = fhi[d];
        n[d] = (long)fhi[d] - flo[d] + 1;
    }
    S.start[0] = 0;
    S.start[1] = 2 * (n[0] + 2) * (n[1] + 2);
    S.start[2] = S.start[1] + 2 * (n[0] + 2) * n[2];
    S.start[3] = S.start[2] + 2 * n[1] * n[2];
    prof_begin(prof, "k_phi_cf_bc", stream);
    hipLaunchKernelGGL(k_phi_cf_bc, dim3((unsigned)((S.start[3] + 255) / 256)), dim3(256), 0, stream, F, O, N, S, 1.0 - a, a);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

// The coarse-fine boundary values of a level that is a union of boxes, into the face array X of its plan: thread t takes the
// face r = t / zones (x low, x high, y low, ...) of the zone t % zones of the bounding box L; a covered zone whose flag of that
// face is set writes k_phi_cf_bc's value of the face zone -- its uncovered neighbour -- into the slot of the face.  A face between
// two boxes of the level, and every other slot of X, is not written.
__global__ void __launch_bounds__(256) k_phi_cf_boxes(DFab X, DFab O, DFab N, MgLevel L, const unsigned char* __restrict__ flags,
                                                     double oma, double a)
{
    const long zones = (long)L.n[0] * L.n[1] * L.n[2];
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 6 * zones) return;
    const int r = (int)(t / zones);
    const long q = t % zones;
    const int d = r >> 1, side = r & 1;
    if (!(flags[q] & MGF_COVERED) || !(flags[q] & mgf_face(d, side))) return;
    const long rr = q / L.n[0];
    const int z[3] = { L.lo[0] + (int)(q % L.n[0]), L.lo[1] + (int)(rr % L.n[1]), L.lo[2] + (int)(rr / L.n[1]) };
    int g[3] = { z[0], z[1], z[2] }, f[3] = { z[0], z[1], z[2] };
    g[d] += side ? 1 : -1;
    f[d] += side;
    X.p[mg_at(X, f[0], f[1], f[2]) + X.sn * d] = cf_face_value(O, N, oma, a, d, side, g);
}

int launch_phi_cf_boxes(PoissonPlan* P, const DFab& X, const DFab& O, const DFab& N, double a, hipStream_t stream, Profiler* prof)
{
    const MgLevel& L = P->lev[0];
    const long n = 6 * (long)L.n[0] * L.n[1] * L.n[2];
    prof_begin(prof, "k_phi_cf_boxes", stream);
    hipLaunchKernelGGL(k_phi_cf_boxes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, X, O, N, L,
                       (const unsigned char*)P->flags[0], 1.0 - a, a);
    prof_end(prof, stream);
    return hipGetLastError() == hipSuccess ? 0 : CASTRO_AMD_ERR_HIP;
}

} // namespace cad
