// probe_sources.cpp -- the reference's source-term functions added after the hydro path (Source/sources/Castro_sponge.cpp,
// Source/gravity/Castro_gravity.cpp, Source/gravity/Castro_pointmass.cpp, compiled UNMODIFIED and IN PLACE from the reference
// tree against the stand-in headers): Castro::apply_sponge and construct_new_sponge_source, construct_old/new_gravity_source
// for grav_source_type 1-4, Castro::pointmass_update.  Only this driver is ours.  STUB-COMPILED, NOT oracle/_ref.
//
// pointmass_update on several boxes: every box is run as one rank would run it.  The stand-in of
// ParallelDescriptor::ReduceRealSum hands the box's own sum to the probe; pass 1 records it and answers 0 (no restore), the
// probe adds the parts in box order, and pass 2 answers with that total, so the reference's own `> 0` test and restore run on
// every box with the number all ranks would hold.
#include <Castro.H>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <vector>

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
    if (!ok) { std::fprintf(stderr, "probe_sources: %s\n", what.c_str()); std::exit(3); }
}

// dx, problo, center of a case; the domain is not read by the three files
static void set_geometry(const std::string& P)
{
    for (int d = 0; d < 3; ++d) {
        Castro::geom.d.prob_lo[d] = in[P + "problo"][d];
        Castro::geom.d.dx[d] = in[P + "dx"][d];
        Castro::geom.d.prob_hi[d] = in[P + "problo"][d] + 64 * in[P + "dx"][d];
        Castro::geom.d.domain.lo_[d] = 0; Castro::geom.d.domain.hi_[d] = 63;
        problem::center[d] = in[P + "center"][d];
    }
}

static long zones(const int* lo, const int* hi) { return (long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1); }

static void box_of(const Arr& a, int off, int* lo, int* hi)
{
    for (int d = 0; d < 3; ++d) { lo[d] = (int)a[off + d]; hi[d] = (int)a[off + 3 + d]; }
}

static double scalar(const std::string& key) { need(in.count(key) == 1, "missing " + key); return in[key][0]; }

static void sponge_cases(Castro& c)
{
    for (int cfg = 0; cfg < 64; ++cfg) {
        const std::string P = "sponge" + std::to_string(cfg) + ".";
        if (!in.count(P + "box")) continue;
        set_geometry(P);
        int lo[3], hi[3];
        box_of(in[P + "box"], 0, lo, hi);
        castro::do_sponge = 1;
        castro::sponge_lower_radius = scalar(P + "lower_radius");     castro::sponge_upper_radius = scalar(P + "upper_radius");
        castro::sponge_lower_density = scalar(P + "lower_density");   castro::sponge_upper_density = scalar(P + "upper_density");
        castro::sponge_lower_pressure = scalar(P + "lower_pressure"); castro::sponge_upper_pressure = scalar(P + "upper_pressure");
        castro::sponge_lower_factor = scalar(P + "lower_factor");     castro::sponge_upper_factor = scalar(P + "upper_factor");
        castro::sponge_target_x_velocity = in[P + "target_velocity"][0];
        castro::sponge_target_y_velocity = in[P + "target_velocity"][1];
        castro::sponge_target_z_velocity = in[P + "target_velocity"][2];
        castro::sponge_timescale = scalar(P + "timescale");
        castro::sponge_implicit = (int)scalar(P + "implicit");
        stub_eos::gamma = scalar(P + "eos_gamma");
        const double dt = scalar(P + "dt");
        const long nz = zones(lo, hi);
        const Box bx(lo, hi);
        Arr U = in[P + "U"];
        need((long)U.size() == NUM_STATE * nz, P + "U has the wrong size");
        Arr S1((size_t)NSRC * nz, 0.0), S2((size_t)NSRC * nz, 0.0);
        c.apply_sponge(bx, Array4<Real const>(U.data(), lo, hi, NUM_STATE), Array4<Real>(S1.data(), lo, hi, NSRC), dt);
        MultiFab state(U.data(), bx, NUM_STATE), source(S2.data(), bx, NSRC);
        c.construct_new_sponge_source(source, state, state, 0.0, dt);
        need(std::memcmp(S1.data(), S2.data(), 8 * S1.size()) == 0, P + ": apply_sponge and construct_new_sponge_source differ");
        out[P + "src"] = S2;
        castro::do_sponge = 0;
    }
}

static void gravity_cases(Castro& c)
{
    for (int cfg = 0; cfg < 64; ++cfg) {
        const std::string P = "grav" + std::to_string(cfg) + ".";
        if (!in.count(P + "box")) continue;
        set_geometry(P);
        int lo[3], hi[3], glo[3], ghi[3];
        box_of(in[P + "box"], 0, lo, hi);
        for (int d = 0; d < 3; ++d) { glo[d] = lo[d] - 1; ghi[d] = hi[d] + 1; }
        castro::do_grav = 1;
        castro::grav_source_type = (int)scalar(P + "grav_source_type");
        const double dt = scalar(P + "dt");
        const long nz = zones(lo, hi), ng = zones(glo, ghi);
        const Box bx(lo, hi), gbx(glo, ghi);
        Arr Uold = in[P + "uold"], Unew = in[P + "unew"], Gold = in[P + "gold"], Gnew = in[P + "gnew"];
        need((long)Uold.size() == NUM_STATE * nz && (long)Unew.size() == NUM_STATE * nz, P + "uold / unew have the wrong size");
        need((long)Gold.size() == 3 * ng && (long)Gnew.size() == 3 * ng, P + "gold / gnew have the wrong size");
        Arr PHI((size_t)ng, 0.0), VOL((size_t)nz, in[P + "dx"][0] * in[P + "dx"][1] * in[P + "dx"][2]);
        Arr S1((size_t)NSRC * nz, 0.0), S2((size_t)NSRC * nz, 0.0);
        MultiFab uold(Uold.data(), bx, NUM_STATE), unew(Unew.data(), bx, NUM_STATE), gold(Gold.data(), gbx, 3), gnew(Gnew.data(), gbx, 3),
                 phi(PHI.data(), gbx, 1), s1(S1.data(), bx, NSRC), s2(S2.data(), bx, NSRC);
        c.old_data[Gravity_Type] = &gold; c.new_data[Gravity_Type] = &gnew;
        c.old_data[PhiGrav_Type] = &phi;  c.new_data[PhiGrav_Type] = &phi;
        c.old_data[State_Type] = &uold;   c.new_data[State_Type] = &unew;
        c.volume = MultiFab(VOL.data(), bx, 1);
        Arr F[3];
        c.mass_fluxes.clear();
        for (int d = 0; d < 3; ++d) {
            F[d] = in[P + "mflux" + std::to_string(d)];
            int fhi[3];
            for (int e = 0; e < 3; ++e) fhi[e] = hi[e] + (e == d ? 1 : 0);
            need((long)F[d].size() == zones(lo, fhi), P + "mflux has the wrong size");
            c.mass_fluxes.emplace_back(new MultiFab(F[d].data(), Box(lo, fhi), 1));
        }
        c.construct_old_gravity_source(s1, uold, 0.0, dt);
        c.construct_new_gravity_source(s2, uold, unew, 0.0, dt);
        out[P + "old"] = S1; out[P + "new"] = S2;
        c.mass_fluxes.clear();
        castro::do_grav = 0;
    }
}

static double pm_part, pm_total;
static void pm_record_and_answer_zero(Real& x) { pm_part = x; x = 0.0; }
static void pm_answer_total(Real& x) { x = pm_total; }

static void pointmass_cases(Castro& c)
{
    Amr amr;
    c.parent = &amr;
    for (int cfg = 0; cfg < 64; ++cfg) {
        const std::string P = "pm" + std::to_string(cfg) + ".";
        if (!in.count(P + "boxes")) continue;
        set_geometry(P);
        amr.finest_level = 1; c.level = 1;                               // the finest level: the update runs
        castro::point_mass_fix_solution = 1;
        const Arr& B = in[P + "boxes"];
        const int nbox = (int)(B.size() / 6);
        const double vol = in[P + "dx"][0] * in[P + "dx"][1] * in[P + "dx"][2], mass0 = scalar(P + "mass");
        std::vector<Arr> So(nbox), Sn(nbox);
        Arr parts;
        for (int pass = 0; pass < 2; ++pass) {
            ParallelDescriptor::sum_over_ranks() = pass == 0 ? pm_record_and_answer_zero : pm_answer_total;
            for (int b = 0; b < nbox; ++b) {
                int lo[3], hi[3];
                box_of(B, 6 * b, lo, hi);
                const long nz = zones(lo, hi);
                if (pass == 0) {
                    So[b] = in[P + "sold" + std::to_string(b)]; Sn[b] = in[P + "snew" + std::to_string(b)];
                    need((long)So[b].size() == NUM_STATE * nz && (long)Sn[b].size() == NUM_STATE * nz, P + "sold / snew have the wrong size");
                }
                Arr VOL((size_t)nz, vol);
                const Box bx(lo, hi);
                MultiFab sold(So[b].data(), bx, NUM_STATE), snew(Sn[b].data(), bx, NUM_STATE);
                c.old_data[State_Type] = &sold; c.new_data[State_Type] = &snew;
                c.volume = MultiFab(VOL.data(), bx, 1);
                castro::point_mass = mass0;
                c.pointmass_update(0.0, 1.0);
                if (pass == 0) {
                    need(std::memcmp(Sn[b].data(), in[P + "snew" + std::to_string(b)].data(), 8 * Sn[b].size()) == 0, P + ": pass 1 wrote S_new");
                    parts.push_back(pm_part);
                } else {
                    out[P + "snew" + std::to_string(b)] = Sn[b];
                    if (b == 0) out[P + "mass"] = Arr(1, castro::point_mass);
                    else need(out[P + "mass"][0] == castro::point_mass, P + ": the ranks disagree about the point mass");
                }
            }
            if (pass == 0) {
                pm_total = 0.0;
                for (double x : parts) pm_total += x;
                out[P + "parts"] = parts; out[P + "delta"] = Arr(1, pm_total);
            }
        }
        ParallelDescriptor::sum_over_ranks() = nullptr;
        castro::point_mass_fix_solution = 0;
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    read_blob(argv[1]);
    Castro castro_obj;
    Gravity gravity_obj;
    castro_obj.gravity = &gravity_obj;
    sponge_cases(castro_obj);
    gravity_cases(castro_obj);
    pointmass_cases(castro_obj);
    write_blob(argv[2]);
    return 0;
}
