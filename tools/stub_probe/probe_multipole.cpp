// probe_multipole.cpp -- calls calcLegPolyL, calcAssocLegPolyLM and multipole_add of the reference's Source/gravity/Gravity_util.H,
// included unmodified and in place, on seeded zones.  Compiled with -DPROBE_MULTIPOLE against the stand-in headers of stub/
// (tools/stub_probe/README.md); the recipe is make_multipole_vectors.py.  NOT a reference build.
//
// Stand-ins (here and in stub/AMReX_Stub.H, behind PROBE_MULTIPOLE only): gravity::lnum, the multipole:: globals the header
// names, problem::center, C::Gconst, amrex::Gpu::Handler and a serial amrex::Gpu::deviceReduceSum.  factArray holds
// 2 (l - m)! / (l + m)! over the header's own factorial(); volumeFactor and the parity factors are 1 (no Symmetry face).
//
// in:  nz, then nz records (cosTheta, phiAngle, r, rho, vol)                                        -- doubles
// out: for lnum = 0, 2, 6 and every zone: legPolyL(l), l = 0 .. lnum; assocLegPolyLM(l, m) over the reference's loop nest
//      (m = 1 .. lnum outer, l = 1 .. lnum inner, m <= l), zero elsewhere, (lnum + 1)^2 entries [l][m]; then what ONE call of
//      multipole_add(..., npts = 1, nlo = 0, index = 0, handler, parity = true) adds to zeroed qL0 (lnum + 1), qLC and qLS
//      ((lnum + 1)^2 each, [l][m])
#ifndef PROBE_MULTIPOLE
#error "compile with -DPROBE_MULTIPOLE"
#endif
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "AMReX_Stub.H"

using namespace amrex;

// what Gravity_util.H names and does not declare; only the first five are read by the functions called here
namespace gravity { int lnum = 0; }
namespace multipole {
    const int MAXL = 6;                                       // the largest order probed
    Array2D<Real, 0, MAXL, 0, MAXL> factArray;                // 2 (l - m)! / (l + m)!
    Array1D<Real, 0, MAXL> parity_q0;                         // 1: no Symmetry face
    Array2D<Real, 0, MAXL, 0, MAXL> parity_qC_qS;             // 1
    Real volumeFactor = 1.0;
    Real rmax = 1.0;                                          // multipole_symmetric_add (never called)
    Array1D<bool, 0, 2> doSymmetricAddLo;                     // multipole_symmetric_add (never called)
}
namespace problem { Real center[3] = {0.0, 0.0, 0.0}; }      // multipole_symmetric_add
namespace C { const Real Gconst = 6.67428e-8; }              // the direct-sum functions (never called)

#include "Gravity_util.H"

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 2;
    double head = 0.0;
    if (std::fread(&head, sizeof(double), 1, fi) != 1) return 2;
    const int nz = (int)head;
    std::vector<double> in((size_t)nz * 5);
    if (std::fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);

    // the factors multipole_add multiplies with, for a domain without Symmetry faces: the parity factors are 1 and
    // factArray(l, m) = 2 (l - m)! / (l + m)! for 1 <= m <= l, with the header's own factorial()
    for (int l = 0; l <= multipole::MAXL; ++l) {
        multipole::parity_q0(l) = 1.0;
        for (int m = 0; m <= multipole::MAXL; ++m) {
            multipole::parity_qC_qS(l, m) = 1.0;
            Real f = 0.0;
            if (m >= 1 && m <= l) { f = 2.0 * factorial(l - m); f /= factorial(l + m); }
            multipole::factArray(l, m) = f;
        }
    }

    std::vector<double> out;
    const int lnums[3] = {0, 2, 6};
    for (int c = 0; c < 3; ++c) {
        const int lnum = lnums[c], n1 = lnum + 1;
        gravity::lnum = lnum;
        for (int z = 0; z < nz; ++z) {
            const Real cosTheta = in[5 * z], phiAngle = in[5 * z + 1], r = in[5 * z + 2], rho = in[5 * z + 3], vol = in[5 * z + 4];
            Real legPolyL = 0.0, legPolyL1 = 0.0, legPolyL2 = 0.0;
            for (int l = 0; l <= lnum; ++l) {
                calcLegPolyL(l, legPolyL, legPolyL1, legPolyL2, cosTheta);
                out.push_back(legPolyL);
            }
            std::vector<double> assoc((size_t)n1 * n1, 0.0);
            Real a = 0.0, a1 = 0.0, a2 = 0.0;
            for (int m = 1; m <= lnum; ++m) {
                for (int l = 1; l <= lnum; ++l) {
                    if (m > l) continue;
                    calcAssocLegPolyLM(l, m, a, a1, a2, cosTheta);
                    assoc[(size_t)l * n1 + m] = a;
                }
            }
            out.insert(out.end(), assoc.begin(), assoc.end());
            // the moment arrays as fill_multipole_BCs boxes them: (l, m, n) with one radial bin
            const int lo[3] = {0, 0, 0}, hi0[3] = {lnum, 0, 0}, hiC[3] = {lnum, lnum, 0};
            std::vector<double> q0((size_t)n1, 0.0), qC((size_t)n1 * n1, 0.0), qS((size_t)n1 * n1, 0.0);
            std::vector<double> u0((size_t)n1, 0.0), uC((size_t)n1 * n1, 0.0), uS((size_t)n1 * n1, 0.0);
            Array4<Real> qL0(q0.data(), lo, hi0, 1), qLC(qC.data(), lo, hiC, 1), qLS(qS.data(), lo, hiC, 1);
            Array4<Real> qU0(u0.data(), lo, hi0, 1), qUC(uC.data(), lo, hiC, 1), qUS(uS.data(), lo, hiC, 1);
            amrex::Gpu::Handler handler;
            multipole_add(cosTheta, phiAngle, r, rho, vol, qL0, qLC, qLS, qU0, qUC, qUS, 1, 0, 0, handler, true);
            for (int l = 0; l <= lnum; ++l) out.push_back(qL0(l, 0, 0));
            for (int l = 0; l <= lnum; ++l) for (int m = 0; m <= lnum; ++m) out.push_back(qLC(l, m, 0));
            for (int l = 0; l <= lnum; ++l) for (int m = 0; m <= lnum; ++m) out.push_back(qLS(l, m, 0));
            for (double v : u0) if (v != 0.0) { std::fprintf(stderr, "the upper moments must stay zero\n"); return 3; }
        }
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), fo);
    std::fclose(fo);
    return 0;
}
