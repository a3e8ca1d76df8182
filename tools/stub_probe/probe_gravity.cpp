// probe_gravity.cpp -- calls the reference's own Gravity::install_level, compute_radial_mass, make_radial_gravity,
// interpolate_monopole_grav, add_pointmass_to_gravity, init_multipole_grav and fill_multipole_BCs on seeded inputs.  The member
// functions are compiled UNMODIFIED but NOT IN PLACE: make_gravity_vectors.py slices their verbatim text out of the reference's
// Source/gravity/Gravity.cpp into a translation unit in a temporary directory (that file pulls in MLMG, MLPoisson and
// FillPatchUtil through its other members), behind #include lines for the stand-ins and for the reference's own Gravity.H and
// Gravity_util.H, which are included unmodified and in place.  Only this driver, the constructor and the definitions of the
// file-scope variables of Gravity.cpp are ours; none of them holds arithmetic of the functions under test.
// Compiled with -DPROBE_GRAVITY and without OpenMP, so the loop nest (k, j, i, kk, jj, ii) fixes the order of every sum.
// STUB-COMPILED, NOT oracle/_ref (tools/stub_probe/README.md).
//
// in / out: named arrays of doubles (the blob format of probe_sources.cpp).  Families rm<c>. (compute_radial_mass),
// rg<c>. (install_level + make_radial_gravity), ig<c>. (interpolate_monopole_grav), pg<c>. (add_pointmass_to_gravity),
// mp<c>. (init_multipole_grav + fill_multipole_BCs); the keys are listed where each family is run.
#ifndef PROBE_GRAVITY
#error "compile with -DPROBE_GRAVITY"
#endif
#include <Castro_GravityProbe.H>
#include <Gravity.H>
#ifdef STUB_GRAVITY_H
#error "the reference's Gravity.H must come first on the include path, not the stand-in of probe_sources.cpp"
#endif
#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>

// ---- the file-scope variables of Gravity.cpp (its lines 26-63) and the run-time parameters ------------------------------------
int Gravity::test_solves = 0;
int Gravity::stencil_type = 0;
Real Gravity::max_radius_all_in_domain = 0.0;
Real Gravity::mass_offset = 0.0;
Real multipole::volumeFactor;
Real multipole::parityFactor;
Real multipole::rmax;
Array1D<bool, 0, 2> multipole::doSymmetricAddLo;
Array1D<bool, 0, 2> multipole::doSymmetricAddHi;
bool multipole::doSymmetricAdd;
Array1D<bool, 0, 2> multipole::doReflectionLo;
Array1D<bool, 0, 2> multipole::doReflectionHi;
Array2D<Real, 0, multipole::lnum_max, 0, multipole::lnum_max> multipole::factArray;
Array1D<Real, 0, multipole::lnum_max> multipole::parity_q0;
Array2D<Real, 0, multipole::lnum_max, 0, multipole::lnum_max> multipole::parity_qC_qS;
namespace gravity { std::string gravity_type = "MonopoleGrav"; int drdxfac = 1, lnum = 0, verbose = 0; Real const_grav = 0.0; }
namespace problem { Real center[3] = {0.0, 0.0, 0.0}; }
namespace castro { Real point_mass = 0.0; }

// the constructor without read_params(), make_mg_bc() and the call of init_multipole_grav() (the probe calls that itself)
Gravity::Gravity(Amr* Parent, int _finest_level, BCRec* _phys_bc, int _Density)
    : parent(Parent), LevelData(MAX_LEV), grad_phi_curr(MAX_LEV), grad_phi_prev(MAX_LEV), grids(Parent->boxArray()),
      dmap(Parent->DistributionMap()), abs_tol(MAX_LEV), rel_tol(MAX_LEV), level_solver_resnorm(MAX_LEV), max_rhs(0.0),
      volume(MAX_LEV), area(MAX_LEV), Density(_Density), finest_level(_finest_level), finest_level_allocated(-1), phys_bc(_phys_bc),
      numpts_at_level(0)
{
    radial_grav_old.resize(MAX_LEV);
    radial_grav_new.resize(MAX_LEV);
    radial_mass.resize(MAX_LEV);
    radial_vol.resize(MAX_LEV);
}
Gravity::~Gravity() {}

using Arr = std::vector<double>;
static std::map<std::string, Arr> in, out;

static void read_blob(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    while (f) {
        char name[48];
        int64_t n;
        if (!f.read(name, 48)) break;
        f.read(reinterpret_cast<char*>(&n), 8);
        Arr a((size_t)n);
        f.read(reinterpret_cast<char*>(a.data()), 8 * n);
        in[std::string(name)] = a;
    }
}

static void write_blob(const char* path)
{
    std::ofstream f(path, std::ios::binary);
    for (auto& kv : out) {
        char name[48] = {0};
        std::strncpy(name, kv.first.c_str(), 47);
        int64_t n = (int64_t)kv.second.size();
        f.write(name, 48);
        f.write(reinterpret_cast<const char*>(&n), 8);
        f.write(reinterpret_cast<const char*>(kv.second.data()), 8 * n);
    }
}

static void need(bool ok, const std::string& what)
{
    if (!ok) { std::fprintf(stderr, "probe_gravity: %s\n", what.c_str()); std::exit(3); }
}
static const Arr& arr(const std::string& key) { need(in.count(key) == 1, "missing " + key); return in[key]; }
static double scalar(const std::string& key) { return arr(key)[0]; }
static bool has(const std::string& key) { return in.count(key) == 1; }
static std::string S(int v) { return std::to_string(v); }

// ---- the stand-in hierarchy: levels 0 .. nlev - 1, ratio 2 (or the same zones on every level: `flat`, which lets a function be
//      called with level > 0, where the reference drops what lies beyond the last bin instead of aborting) ------------------------
struct Hier {
    Amr amr;
    BCRec bc;
    std::vector<std::unique_ptr<Castro> > lev;
    std::vector<std::unique_ptr<MultiFab> > vol, sold, snew;
    std::unique_ptr<Gravity> g;
    int nlev = 0;
};

static BoxArray boxes_of(const Arr& a)
{
    BoxArray ba;
    for (size_t b = 0; b + 6 <= a.size(); b += 6) {
        int lo[3], hi[3];
        for (int d = 0; d < 3; ++d) { lo[d] = (int)a[b + d]; hi[d] = (int)a[b + 3 + d]; }
        ba.b.push_back(Box(lo, hi));
    }
    return ba;
}

// the values of component `comp` of every box of `mf` from the arrays key<b> (each on the box of its FAB, ghost zones included)
static void fill_comp(MultiFab& mf, int comp, const std::string& key)
{
    for (size_t b = 0; b < mf.fabs.size(); ++b) {
        const Arr& a = arr(key + S((int)b));
        const long n = mf.fabs[b].box().numPts();
        need((long)a.size() == n, key + S((int)b) + " has the wrong size");
        std::memcpy(mf.fabs[b].dataPtr() + comp * n, a.data(), 8 * n);
    }
}
static void fill_all(MultiFab& mf, Real v) { for (auto& f : mf.fabs) f.setVal<RunOn::Device>(v); }
static void record(const MultiFab& mf, const std::string& key)
{
    for (size_t b = 0; b < mf.fabs.size(); ++b)
        out[key + S((int)b)] = Arr(mf.fabs[b].dataPtr(), mf.fabs[b].dataPtr() + mf.fabs[b].size());
}

static void build(Hier& h, const std::string& P, const std::string& gravity_type)
{
    h.nlev = (int)scalar(P + "nlev");
    const bool flat = has(P + "flat");
    gravity::gravity_type = gravity_type;
    gravity::drdxfac = has(P + "drdxfac") ? (int)scalar(P + "drdxfac") : 1;
    for (int d = 0; d < 3; ++d) {
        problem::center[d] = arr(P + "center")[d];
        h.bc.l[d] = Outflow; h.bc.h[d] = Outflow;
    }
    h.amr.finest_level = h.nlev - 1;
    for (int l = 0; l < h.nlev; ++l) {
        Geometry gm;
        const int r = flat ? 1 : (1 << l);
        for (int d = 0; d < 3; ++d) {
            gm.d.prob_lo[d] = arr(P + "problo")[d];
            gm.d.prob_hi[d] = arr(P + "probhi")[d];
            gm.d.dx[d] = arr(P + "dx")[d] / (double)r;                     // a power of two: exact
            gm.d.domain.lo_[d] = (int)arr(P + "domain")[d] * r;
            gm.d.domain.hi_[d] = ((int)arr(P + "domain")[3 + d] + 1) * r - 1;
        }
        h.amr.geoms.push_back(gm);
        h.amr.ratios.push_back(IntVect(2, 2, 2));
        h.amr.grids.push_back(boxes_of(arr(P + "boxes" + S(l))));
        h.amr.dmaps.push_back(DistributionMapping());
    }
    h.g.reset(new Gravity(&h.amr, h.nlev - 1, &h.bc, URHO));
    for (int l = 0; l < h.nlev; ++l) {
        const BoxArray& ba = h.amr.grids[l];
        h.lev.emplace_back(new Castro);
        Castro& c = *h.lev.back();
        c.geom = h.amr.geoms[l]; c.grids = ba;
        c.state.resize(1);
        c.state[0].t_old = has(P + "t_old" + S(l)) ? scalar(P + "t_old" + S(l)) : 0.0;
        c.state[0].t_new = has(P + "t_new" + S(l)) ? scalar(P + "t_new" + S(l)) : 1.0;
        h.vol.emplace_back(new MultiFab(ba, DistributionMapping(), 1, 0));
        const Real* dx = c.geom.CellSize();
        fill_all(*h.vol.back(), dx[0] * dx[1] * dx[2]);                  // Geometry::GetVolume of a Cartesian level
        // the state: only URHO is read; every other component holds a few-bit value
        h.sold.emplace_back(new MultiFab(ba, DistributionMapping(), NUM_STATE, 0));
        h.snew.emplace_back(new MultiFab(ba, DistributionMapping(), NUM_STATE, 0));
        fill_all(*h.sold.back(), 0.5);
        fill_all(*h.snew.back(), 0.25);
        const std::string l_ = S(l) + "_";
        if (has(P + "rho_old" + l_ + "0")) {
            fill_comp(*h.sold.back(), URHO, P + "rho_old" + l_);
            fill_comp(*h.snew.back(), URHO, P + "rho_new" + l_);
        } else if (has(P + "rho" + l_ + "0")) {
            fill_comp(*h.sold.back(), URHO, P + "rho" + l_);
            fill_comp(*h.snew.back(), URHO, P + "rho" + l_);
        }
        c.old_data.assign(1, h.sold.back().get());
        c.new_data.assign(1, h.snew.back().get());
        h.amr.levels.push_back(&c);
        if (l > 0 && has(P + "mask" + S(l - 1) + "_0")) {                 // the mask of level l - 1, served by level l
            c.fine_mask.define(h.amr.grids[l - 1], DistributionMapping(), 1, 0);
            fill_comp(c.fine_mask, 0, P + "mask" + S(l - 1) + "_");
        }
    }
    for (int l = 0; l < h.nlev; ++l) {
        h.g->numpts_at_level = (int)scalar(P + "numpts" + S(l));          // Gravity::set_numpts_in_gravity
        h.g->install_level(l, h.lev[l].get(), *h.vol[l], nullptr);
    }
}

static std::vector<std::string> cases(const std::string& family)
{
    std::vector<std::string> r;
    for (int c = 0; c < 256; ++c) {
        const std::string P = family + S(c) + ".";
        if (has(P + "nlev")) r.push_back(P);
    }
    return r;
}

// rm<c>.: dx, problo, probhi, center, domain, drdxfac, nlev, flat, level, n1d, boxes<l>, numpts<l>, rho<l>_<b>
//   -> mass, vol (n1d each): compute_radial_mass over the boxes of `level`, in box order, into zeroed arrays
static void radial_mass_cases()
{
    for (const std::string& P : cases("rm")) {
        Hier h;
        build(h, P, "MonopoleGrav");
        const int level = (int)scalar(P + "level"), n1d = (int)scalar(P + "n1d");
        RealVector mass(n1d, 0.0), vol(n1d, 0.0);
        MultiFab& Sn = *h.snew[level];
        for (MFIter mfi(Sn); mfi.isValid(); ++mfi)
            h.g->compute_radial_mass(mfi.tilebox(), Sn[mfi].array(), mass, vol, n1d, level);
        out[P + "mass"] = Arr(mass.begin(), mass.end());
        out[P + "vol"] = Arr(vol.begin(), vol.end());
    }
}

// rg<c>.: as rm, and level, time, t_old<l>, t_new<l>, rho_old<l>_<b>, rho_new<l>_<b>, mask<l>_<b>
//   -> n1d (per level), maxrad, mass<l>, vol<l> (what make_radial_gravity leaves in radial_mass / radial_vol), grav
static void radial_gravity_cases()
{
    for (const std::string& P : cases("rg")) {
        Hier h;
        build(h, P, "MonopoleGrav");
        const int level = (int)scalar(P + "level");
        RealVector rg(h.g->radial_mass[level].size(), std::numeric_limits<Real>::quiet_NaN());
        need(rg.size() == h.g->radial_grav_new[level].size(), "radial_grav is sized as install_level sizes it");
        h.g->make_radial_gravity(level, scalar(P + "time"), rg);
        Arr n1d;
        for (int l = 0; l <= level; ++l) {
            n1d.push_back((double)h.g->radial_mass[l].size());
            out[P + "mass" + S(l)] = Arr(h.g->radial_mass[l].begin(), h.g->radial_mass[l].end());
            out[P + "vol" + S(l)] = Arr(h.g->radial_vol[l].begin(), h.g->radial_vol[l].end());
        }
        out[P + "n1d"] = n1d;
        out[P + "maxrad"] = Arr(1, Gravity::max_radius_all_in_domain);
        out[P + "grav"] = Arr(rg.begin(), rg.end());
        for (double v : rg) need(v == v, P + "every bin of radial_grav is written");
    }
}

// ig<c>.: as rm (flat, level 1), ng, fill, rg (n1d values) -> grav<b>: interpolate_monopole_grav onto FABs grown by ng that hold `fill`
static void interpolate_cases()
{
    for (const std::string& P : cases("ig")) {
        Hier h;
        build(h, P, "MonopoleGrav");
        const int level = (int)scalar(P + "level");
        need(level > 0, "level 0 aborts beyond the last bin");
        const Arr& a = arr(P + "rg");
        RealVector rg(a.begin(), a.end());
        MultiFab grav(h.amr.grids[level], DistributionMapping(), 3, (int)scalar(P + "ng"));
        fill_all(grav, scalar(P + "fill"));
        h.g->interpolate_monopole_grav(level, rg, grav);
        record(grav, P + "grav");
    }
}

// pg<c>.: as rm (one level), mass, ng_grav, ng_phi, grav<b> (3 components on the grown box), phi<b> -> grav<b>, phi<b>
static void pointmass_cases()
{
    for (const std::string& P : cases("pg")) {
        Hier h;
        build(h, P, "MonopoleGrav");
        const BoxArray& ba = h.amr.grids[0];
        MultiFab grav(ba, DistributionMapping(), 3, (int)scalar(P + "ng_grav")), phi(ba, DistributionMapping(), 1, (int)scalar(P + "ng_phi"));
        for (int n = 0; n < 3; ++n) fill_comp(grav, n, P + "grav" + S(n) + "_");
        fill_comp(phi, 0, P + "phi");
        castro::point_mass = scalar(P + "mass");
        h.g->add_pointmass_to_gravity(0, phi, grav, castro::point_mass);
        record(grav, P + "grav");
        record(phi, P + "phi");
    }
}

// the moments are local to fill_multipole_BCs; its three ReduceRealSum calls (qL0, qLC, qLS, in that order, after the zone
// loop) hand them to the probe
static std::vector<Arr> reduced;
static void take_moments(Real* p, int n) { reduced.push_back(Arr(p, p + n)); }

// mp<c>.: as rm, lnum, rho<l>_<b>, mask<l>_<b>, phi<b> (one ghost zone)
//   -> rmax, volumeFactor, parity_q0, parity_qC_qS, symmetric (doSymmetricAdd, the six doSymmetricAddLo/Hi, the six doReflection),
//      factArray ((lnum + 1)^2, [l][m]), npts, qL0 (lnum + 1), qLC, qLS ((lnum + 1)^2, [l][m]) of the outermost bin, vol, phi<b>
static void multipole_cases()
{
    for (const std::string& P : cases("mp")) {
        Hier h;
        build(h, P, "PoissonGrav");
        const int lnum = (int)scalar(P + "lnum"), n1 = lnum + 1;
        gravity::lnum = lnum;
        h.g->init_multipole_grav();
        const int npts = (int)scalar(P + "numpts0");
        h.g->numpts_at_level = npts;
        std::vector<std::unique_ptr<MultiFab> > rhs;
        Vector<MultiFab*> Rhs;
        for (int l = 0; l < h.nlev; ++l) {
            rhs.emplace_back(new MultiFab(h.amr.grids[l], DistributionMapping(), 1, 0));
            fill_comp(*rhs.back(), 0, P + "rho" + S(l) + "_");
            Rhs.push_back(rhs.back().get());
        }
        MultiFab phi(h.amr.grids[0], DistributionMapping(), 1, 1);
        fill_comp(phi, 0, P + "phi");
        reduced.clear();
        ParallelDescriptor::reduce_hook() = take_moments;
        h.g->fill_multipole_BCs(0, h.nlev - 1, Rhs, phi);
        ParallelDescriptor::reduce_hook() = nullptr;
        need(reduced.size() == 3, "three reductions: qL0, qLC, qLS");
        need((int)reduced[0].size() == n1 * npts && (int)reduced[1].size() == n1 * n1 * npts, "the moment arrays are (l, m, bin)");
        // FArrayBox layout: l fastest, then m, then the bin; only the outermost bin is filled (boundary_only)
        Arr q0(n1), qC((size_t)n1 * n1), qS((size_t)n1 * n1), fa((size_t)n1 * n1), pq0(n1), pqc((size_t)n1 * n1);
        for (int n = 0; n < npts - 1; ++n)
            for (int i = 0; i < n1; ++i) need(reduced[0][(size_t)n * n1 + i] == 0.0, "an inner bin of qL0 is not zero");
        for (int l = 0; l <= lnum; ++l) {
            q0[l] = reduced[0][(size_t)(npts - 1) * n1 + l];
            pq0[l] = multipole::parity_q0(l);
            for (int m = 0; m <= lnum; ++m) {
                qC[(size_t)l * n1 + m] = reduced[1][((size_t)(npts - 1) * n1 + m) * n1 + l];
                qS[(size_t)l * n1 + m] = reduced[2][((size_t)(npts - 1) * n1 + m) * n1 + l];
                fa[(size_t)l * n1 + m] = multipole::factArray(l, m);
                pqc[(size_t)l * n1 + m] = multipole::parity_qC_qS(l, m);
            }
        }
        Arr sym(1, multipole::doSymmetricAdd ? 1.0 : 0.0);
        for (int d = 0; d < 3; ++d) sym.push_back(multipole::doSymmetricAddLo(d) ? 1.0 : 0.0);
        for (int d = 0; d < 3; ++d) sym.push_back(multipole::doSymmetricAddHi(d) ? 1.0 : 0.0);
        for (int d = 0; d < 3; ++d) sym.push_back(multipole::doReflectionLo(d) ? 1.0 : 0.0);
        for (int d = 0; d < 3; ++d) sym.push_back(multipole::doReflectionHi(d) ? 1.0 : 0.0);
        out[P + "rmax"] = Arr(1, multipole::rmax);
        out[P + "volumeFactor"] = Arr(1, multipole::volumeFactor);
        out[P + "parity_q0"] = pq0; out[P + "parity_qC_qS"] = pqc; out[P + "symmetric"] = sym; out[P + "factArray"] = fa;
        out[P + "npts"] = Arr(1, (double)npts);
        out[P + "qL0"] = q0; out[P + "qLC"] = qC; out[P + "qLS"] = qS;
        Arr vols;
        for (int l = 0; l < h.nlev; ++l) vols.push_back(h.vol[l]->fabs[0].dataPtr()[0]);
        out[P + "vol"] = vols;
        record(phi, P + "phi");
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    read_blob(argv[1]);
    radial_mass_cases();
    radial_gravity_cases();
    interpolate_cases();
    pointmass_cases();
    multipole_cases();
    write_blob(argv[2]);
    return 0;
}
