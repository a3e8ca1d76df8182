// translation unit of tests/test_ext_bc_cpu.py::test_amrex_adapter_ext_bc_fill_compiles_against_the_api_mock: the adapter's
// ext_bc_fill after its fill_boundary, as a host calls them
#include <castro_hydro_amd_amrex.H>
void use_ext_bc (amrex::MultiFab& state, const amrex::Geometry& g, const amrex::BCRec& bc, const castro_amd_params& p, int* d_unconverged)
{
    castro_amd_ext_bc ext{};
    ext.lo_type[2] = 1;
    ext.const_grav = -1.0;
    castro_amd::fill_boundary(state, g, bc);
    castro_amd::ext_bc_fill(state, g, bc, p, ext);
    castro_amd::ext_bc_fill(state, g, bc, p, ext, d_unconverged);
}
