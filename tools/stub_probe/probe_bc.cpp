// probe_bc.cpp -- the reference's boundary overrides of the state fill (Source/problems/ambient_fill.cpp and
// Source/problems/hse_fill.cpp, compiled UNMODIFIED and IN PLACE from the reference tree against the stand-in headers, with
// -DPROBE_BC -DGRAVITY): ambient_fill, then hse_fill, as ca_statefill (Source/problems/Castro_bc_fill_nd.cpp:41-105) calls them,
// on FABs whose zones outside the domain hold the generic fill already.  Only this driver is ours.  STUB-COMPILED, NOT oracle/_ref.
//
// The BCRec of every component is the one Castro_setup.cpp:40-53 makes of the physical boundary for a scalar: Interior ->
// INT_DIR, Inflow -> EXT_DIR, Outflow -> FOEXTRAP, the walls -> REFLECT_EVEN (the two files read the density's only).
#include <Castro.H>
#include <Castro_bc_fill_nd.H>
#include <ambient.H>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <vector>

namespace ambient { Real ambient_state[NUM_STATE]; }

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

static const Arr& need(const std::string& key, size_t n)
{
    if (in.count(key) != 1 || in[key].size() != n) { std::fprintf(stderr, "probe_bc: %s missing or of the wrong size\n", key.c_str()); std::exit(3); }
    return in[key];
}

static int math_bc(double phys)
{
    switch ((int)phys) {
    case Interior: return INT_DIR;
    case Inflow: return EXT_DIR;
    case Outflow: return FOEXTRAP;
    default: return REFLECT_EVEN;
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    read_blob(argv[1]);
    for (int c = 0; c < 256; ++c) {
        const std::string P = "bc" + std::to_string(c) + ".";
        if (!in.count(P + "box")) continue;
        const Arr& B = need(P + "box", 6);
        int lo[3], hi[3];
        Geometry geom;
        BCRec bc;
        for (int d = 0; d < 3; ++d) {
            lo[d] = (int)B[d]; hi[d] = (int)B[3 + d];
            geom.d.dx[d] = need(P + "dx", 3)[d];
            geom.d.prob_lo[d] = 0.0;
            geom.d.domain.lo_[d] = (int)need(P + "domlo", 3)[d];
            geom.d.domain.hi_[d] = (int)need(P + "domhi", 3)[d];
            geom.d.prob_hi[d] = geom.d.dx[d] * (geom.d.domain.hi_[d] + 1);
            bc.l[d] = math_bc(need(P + "lo_bc", 3)[d]);
            bc.h[d] = math_bc(need(P + "hi_bc", 3)[d]);
        }
        const Arr& T = need(P + "types", 6);
        castro::xl_ext_bc_type = (int)T[0]; castro::xr_ext_bc_type = (int)T[1]; castro::yl_ext_bc_type = (int)T[2];
        castro::yr_ext_bc_type = (int)T[3]; castro::zl_ext_bc_type = (int)T[4]; castro::zr_ext_bc_type = (int)T[5];
        const Arr& F = need(P + "flags", 6);
        castro::hse_zero_vels = (int)F[0]; castro::hse_interp_temp = (int)F[1]; castro::hse_reflect_vels = (int)F[2];
        castro::fill_ambient_bc = (int)F[3]; castro::ambient_fill_dir = (int)F[4]; castro::ambient_outflow_vel = (int)F[5];
        gravity::const_grav = need(P + "const_grav", 1)[0];
        stub_eos::gamma = need(P + "eos_gamma", 1)[0];
        for (int n = 0; n < NUM_STATE; ++n) ambient::ambient_state[n] = need(P + "ambient", NUM_STATE)[n];
        const size_t nz = (size_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
        Arr U = need(P + "U", NUM_STATE * nz);
        const Box bx(lo, hi);
        const Vector<BCRec> bcr(NUM_STATE, bc);
        const Array4<Real> state(U.data(), lo, hi, NUM_STATE);
        ambient_fill(bx, state, geom, bcr);
        hse_fill(bx, state, geom, bcr, 0.0);
        out[P + "U"] = U;
    }
    write_blob(argv[2]);
    return 0;
}
