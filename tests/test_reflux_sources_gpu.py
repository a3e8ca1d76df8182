"""GPU tests of castro.update_sources_after_reflux: the register-to-flux operation (k_fluxreg_to_flux and CASTRO_AMD_OP_FLUXREG_TO_FLUX
of k_fab_ops in castro_amd/csrc/aux_kernels.hip), the re-evaluation stage of the one-pass source kernel k_sources_apply (its instantiation 2, reached as
stage 1 | CASTRO_AMD_SOURCES_AFTER_REFLUX of castro_amd_sources_mf / _ex / _g / _opts: the bare stage 2 stays refused), and the driver
(CastroAmr(update_sources_after_reflux=True)) in its three execution forms against the CPU oracle backend, for both numerics builds.

Tolerances.  The register-to-flux operation is an add and a copy: the same bits in both builds.  Stage 2 against the separate
calls (castro_amd_apply_source_fab with -dt, then stage 1): `exact` the same bits; `contract` 1e-10 of a component's maximum
(the project's rtol: the compiler may contract a * b + c differently in the fused kernel).  Driver: `exact` bit for bit against
the oracle backend in every form, `contract` 1e-10 of a field's maximum."""
import numpy as np
import pytest
import torch

from tests import reflux_sources_ref as R
from tests.util import physical_state

pytestmark = pytest.mark.gpu

RTOL = 1e-10
_CACHE = {}


@pytest.fixture(scope="module", params=["exact", "contract"])
def hydro(request):
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    h = castro_amd.HipHydro(0, numerics=request.param)
    yield h
    h.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sl(box, lo, hi):
    return (slice(None),) + tuple(slice(lo[2 - a] - box[0][2 - a], hi[2 - a] - box[0][2 - a] + 1) for a in range(3))


def _shift(box, sh):
    return tuple(box[0][d] + sh[d] for d in range(3)), tuple(box[1][d] + sh[d] for d in range(3))


# ---- 9. the register-to-flux operation ------------------------------------------------------------------------------------------
BX = ((8, 0, 0), (15, 7, 7))                   # the second coarse box of the drivers' geometry: not at the origin


def _flux_box(d):
    hi = list(BX[1])
    hi[d] += 1
    return BX[0], tuple(hi)


def _face_ops():
    """[(d, region lo, region hi, register box, shift of the flux box)]: for every direction the faces of a fine box at the low
    face of the coarse box (index 8 or 0), inside it, and at its high face (index n + 1 = 16 or 8); and a register at x = 0 that
    reaches the face x = 16 through the periodic boundary (the flux FAB described with its box moved by -16)."""
    ops = []
    for d in range(3):
        t = [x for x in range(3) if x != d]
        for plane, span in ((BX[0][d], (2, 5)), (BX[0][d] + 3, (1, 6)), (BX[1][d] + 1, (2, 5))):
            lo, hi = [0, 0, 0], [0, 0, 0]
            lo[d] = hi[d] = plane
            for x in t:
                lo[x], hi[x] = BX[0][x] + span[0], BX[0][x] + span[1]
            if plane == BX[1][d] + 1 and d == 0:
                continue                        # the wrapped register below writes these faces
            ops.append((d, tuple(lo), tuple(hi), (tuple(lo), tuple(hi)), (0, 0, 0)))
    ops.append((0, (0, 2, 2), (0, 5, 5), ((0, 2, 2), (0, 5, 5)), (-16, 0, 0)))
    return ops


@pytest.mark.parametrize("form", ["plain", "table", "long table"])
@pytest.mark.parametrize("ncomp,mass", [(8, True), (8, False), (1, True)])
def test_register_to_flux_against_numpy(hydro, form, ncomp, mass):
    """flux += reg on the faces of the region and mass_flux = flux(URHO) there, nothing else: flux and mass-flux FABs are NaN
    outside the regions and stay NaN; every orientation, the high face of the box, a shifted (periodic) region, 8 components and
    1, with and without the mass-flux FAB -- the call region by region, a table of up to sixteen operations (the by-value form)
    and a longer one (the device-table form: the list twice over, the second half on FABs of its own).  Bit for bit in both builds."""
    from castro_amd import _lib
    rng = np.random.default_rng(11)
    ops = _face_ops()
    nset = 2 if form == "long table" else 1
    assert (len(ops) * nset > 16) == (form == "long table")
    F, M, want_F, want_M, regs = [], [], [], [], []
    for s in range(nset):
        Fs, Ms = [], []
        for d in range(3):
            fb = _flux_box(d)
            shape = tuple(fb[1][a] - fb[0][a] + 1 for a in (2, 1, 0))
            Fs.append(np.full((ncomp,) + shape, np.nan))
            Ms.append(np.full((1,) + shape, np.nan))
        for d, lo, hi, rbox, sh in ops:
            fb = _shift(_flux_box(d), sh)
            Fs[d][_sl(fb, lo, hi)] = rng.normal(size=Fs[d][_sl(fb, lo, hi)].shape)
        F.append(Fs), M.append(Ms)
        want_F.append([x.copy() for x in Fs]), want_M.append([x.copy() for x in Ms])
        regs.append([rng.normal(size=(ncomp,) + tuple(rbox[1][a] - rbox[0][a] + 1 for a in (2, 1, 0))) for d, lo, hi, rbox, sh in ops])
        for (d, lo, hi, rbox, sh), r in zip(ops, regs[s]):
            fb = _shift(_flux_box(d), sh)
            want_F[s][d][_sl(fb, lo, hi)] += r
            if mass:
                want_M[s][d][_sl(fb, lo, hi)][0] = want_F[s][d][_sl(fb, lo, hi)][0]
    dF = [[_t(x) for x in Fs] for Fs in F]
    dM = [[_t(x) for x in Ms] for Ms in M]
    dR = [[_t(r) for r in rs] for rs in regs]
    specs = []
    for s in range(nset):
        for (d, lo, hi, rbox, sh), r in zip(ops, dR[s]):
            fb = _shift(_flux_box(d), sh)
            if form == "plain":
                hydro.fluxreg_to_flux(dF[s][d], fb, r, rbox, dM[s][d] if mass else None, fb, lo, hi, ncomp)
            else:
                specs.append((_lib.OP_FLUXREG_TO_FLUX, d, ncomp, lo, hi, 0.0, 0.0, (dF[s][d], fb), (r, rbox),
                              (dM[s][d], fb) if mass else None))
    if specs:
        hydro.fab_ops(hydro.make_ops(specs))
    torch.cuda.synchronize()
    for s in range(nset):
        for d in range(3):
            assert np.array_equal(dF[s][d].cpu().numpy(), want_F[s][d], equal_nan=True), (s, d)
            assert np.array_equal(dM[s][d].cpu().numpy(), want_M[s][d], equal_nan=True), (s, d)
            assert np.isfinite(want_F[s][d]).sum() > 0 and (not mass or np.isfinite(want_M[s][d]).sum() > 0)


def test_register_to_flux_argument_checks(hydro):
    """a region outside the flux FAB, the register or the mass-flux FAB, and ncomp beyond a FAB's components, are refused"""
    fb, rbox = _flux_box(0), ((16, 2, 2), (16, 5, 5))
    Fx = torch.zeros((8, 8, 8, 9), dtype=torch.float64, device="cuda")
    Mx = torch.zeros((1, 8, 8, 9), dtype=torch.float64, device="cuda")
    r = torch.zeros((8, 4, 4, 1), dtype=torch.float64, device="cuda")
    hydro.fluxreg_to_flux(Fx, fb, r, rbox, Mx, fb, rbox[0], rbox[1], 8)
    for args in ((Fx, fb, r, rbox, Mx, fb, (17, 2, 2), (17, 5, 5), 8), (Fx, fb, r, rbox, Mx, fb, (16, 1, 2), (16, 5, 5), 8),
                 (Fx, fb, r, rbox, Mx[:, :, :, :8].contiguous(), BX, rbox[0], rbox[1], 8), (Fx, fb, r[:4], rbox, Mx, fb, rbox[0], rbox[1], 8)):
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.fluxreg_to_flux(*args)
    torch.cuda.synchronize()


# ---- 10. stage 2 of the one-pass source kernel ----------------------------------------------------------------------------------
BOXES = [((3, 2, 5), (10, 9, 12)), ((20, 4, 1), (24, 10, 3))]          # 8 x 8 x 8 and 5 x 7 x 3: odd extents, the tail of a workgroup
DT = 0.011


def _stage_case():
    """per box: S_old, the S_new and the stored new-time source a stage-1 call would have left (made below, per build), mass
    fluxes, gravity FABs; then what a reflux does to them -- S_new and the mass fluxes moved a little"""
    if "stage" not in _CACHE:
        rng = np.random.default_rng(23)
        out = []
        for lo, hi in BOXES:
            gb = (tuple(x - 4 for x in lo), tuple(x + 4 for x in hi))
            vb = (tuple(x - 1 for x in lo), tuple(x + 1 for x in hi))
            UO, UN = physical_state(rng, gb[0], gb[1], jump=True), physical_state(rng, gb[0], gb[1], jump=True)
            fb, M = [], []
            for d in range(3):
                fhi = list(hi)
                fhi[d] += 1
                fb.append((lo, tuple(fhi)))
                M.append(rng.normal(size=(1,) + tuple(fhi[a] - lo[a] + 1 for a in (2, 1, 0))))
            g = [rng.uniform(-1.0, 1.0, size=(3,) + tuple(vb[1][a] - vb[0][a] + 1 for a in (2, 1, 0))) for _ in range(2)]
            n = tuple(hi[a] - lo[a] + 1 for a in (2, 1, 0))
            out.append(dict(lo=lo, hi=hi, gb=gb, vb=vb, bx=(lo, hi), UO=UO, UN=UN, fb=fb, M=M, gold=g[0], gnew=g[1],
                            dU=1.0 + 1.e-3 * rng.normal(size=(8,) + n), dM=[1.0 + 1.e-2 * rng.normal(size=m.shape) for m in M]))
        _CACHE["stage"] = out
    return _CACHE["stage"]


def _settings(form):
    from castro_amd import _lib
    sp = _lib.make_sponge(5.e-3, lower_radius=0.3, upper_radius=1.2, lower_density=0.5, upper_density=1.2, center=(0.7, 0.4, 0.3))
    rot = _lib.make_rotation(1.5, center=(0.6, 0.3, 0.2))
    return dict(vector=dict(vec=(0.3, -0.7, -9.8)), rotation=dict(rot=rot), fabs=dict(gfab=True), sponge=dict(sp=sp),
                all_vector=dict(vec=(0.3, -0.7, -9.8), rot=rot, sp=sp), all_fabs=dict(gfab=True, rot=rot, sp=sp))[form]


def _separate_new_sources(h, b, UO, Un, src, M, go, gn, s, geom, P, dt):
    lo, hi, gb = b["lo"], b["hi"], b["gb"]
    src.zero_()
    if s.get("vec") is not None:
        h.new_gravity_source(UO, gb, Un, gb, src, b["bx"], M, b["fb"], lo, hi, s["vec"], 4, dt, geom)
    if s.get("gfab"):
        h.new_gravity_source_gfab(UO, gb, Un, gb, src, b["bx"], M, b["fb"], lo, hi, go, gn, b["vb"], 4, dt, geom)
    if s.get("rot") is not None:
        h.new_rotation_source(UO, gb, Un, gb, src, b["bx"], M, b["fb"], lo, hi, s["rot"], geom, dt)
    if s.get("sp") is not None:
        h.new_sponge_source(Un, gb, src, b["bx"], lo, hi, s["sp"], geom, P, dt)
    h.apply_source(Un, gb, Un, gb, dt, src, b["bx"], 7, lo, hi, P, ntimes=1)


def _one_pass(h, stage, tabs, s, geom, P, dt):
    boxes = h.make_source_boxes([(b["lo"], b["hi"], (UO, b["gb"]), (Un, b["gb"]), (src, sb), M, b["fb"]) for b, UO, Un, src, sb, M, go, gn in tabs])
    kw = {} if s.get("sp") is None else {"sponge": s["sp"]}
    if s.get("gfab"):
        h.sources_mf_g(stage, boxes, h.make_grav_fabs([(go, b["vb"]) for b, UO, Un, src, sb, M, go, gn in tabs]),
                       h.make_grav_fabs([(gn, b["vb"]) for b, UO, Un, src, sb, M, go, gn in tabs]), 4, s.get("rot"), geom, P, dt, ntimes=1, **kw)
    else:
        h.sources_mf(stage, boxes, s.get("vec"), 4, s.get("rot"), geom, P, dt, ntimes=1, **kw)


@pytest.mark.parametrize("form", ["vector", "rotation", "fabs", "sponge", "all_vector", "all_fabs"])
def test_stage_2_equals_the_separate_calls(hydro, form):
    """A level table of two boxes.  Stage 1 by the separate single-box calls leaves S_new and the stored source; a reflux then
    moves S_new and the mass fluxes.  Stage 2 in one launch against castro_amd_apply_source_fab(-dt) + the new-source calls +
    castro_amd_apply_source_fab(+dt) box by box: S_new (whole FAB: ghost zones untouched) and new_source.  Stage 1 of the same
    table on the same inputs is still the separate calls' bits (both builds, as before stage 2 existed)."""
    from castro_amd import _lib
    s, dt = _settings(form), DT
    geom = _lib.make_geom((32, 16, 16), prob_hi=(1.6, 0.8, 0.8))
    P = _lib.default_params()
    sep, one, first = [], [], []
    for b in _stage_case():
        UO, M, go, gn = _t(b["UO"]), [_t(m) for m in b["M"]], _t(b["gold"]), _t(b["gnew"])
        n = tuple(b["hi"][a] - b["lo"][a] + 1 for a in (2, 1, 0))
        # what the advance leaves: stage 1 by separate calls
        Un, src = _t(b["UN"]), torch.zeros((7,) + n, dtype=torch.float64, device="cuda")
        _separate_new_sources(hydro, b, UO, Un, src, M, go, gn, s, geom, P, dt)
        # the same through the table, stage 1
        Un1, src1 = _t(b["UN"]), torch.full((7,) + n, 3.0, dtype=torch.float64, device="cuda")
        first.append((b, UO, Un1, src1, b["bx"], M, go, gn, Un.clone(), src.clone()))
        # the reflux
        v = _sl(b["gb"], b["lo"], b["hi"])
        Un[v] *= _t(b["dU"])
        M2 = [m * _t(x) for m, x in zip(M, b["dM"])]
        Un2, src2 = Un.clone(), src.clone()
        # separate calls: the stored source out, clean, the new sources, apply, clean
        hydro.apply_source(Un, b["gb"], Un, b["gb"], -dt, src, b["bx"], 7, b["lo"], b["hi"], P, ntimes=1)
        _separate_new_sources(hydro, b, UO, Un, src, M2, go, gn, s, geom, P, dt)
        sep.append((Un, src))
        one.append((b, UO, Un2, src2, b["bx"], M2, go, gn))
    _one_pass(hydro, 1, [x[:8] for x in first], s, geom, P, dt)
    _one_pass(hydro, 1 | _lib.SOURCES_AFTER_REFLUX, one, s, geom, P, dt)
    torch.cuda.synchronize()
    for (b, UO, Un1, src1, sb, M, go, gn, Un_want, src_want) in first:
        assert torch.equal(src1, src_want) and torch.equal(Un1, Un_want), "stage 1 of the table"
    for (Un, src), (b, UO, Un2, src2, sb, M2, go, gn) in zip(sep, one):
        assert src.abs().max() > 0.0
        for name, got, want in (("S_new", Un2, Un), ("new_source", src2, src)):
            same = torch.equal(got, want)
            dev = max(float((got[c] - want[c]).abs().max() / want[c].abs().max()) for c in range(want.shape[0]) if want[c].abs().max() > 0)
            print("stage 2 %s %s %s box %s: bitwise %s, max deviation / component maximum %.3g" % (hydro.numerics, form, name, b["bx"], same, dev))
            if hydro.numerics == "exact":
                assert same, "%s: %d entries differ" % (name, int((got != want).sum()))
            else:
                assert dev <= RTOL


def test_stage_0_of_a_table_is_unchanged(hydro):
    """stage 0 on the two-box table against the single-box entry points (old gravity + old rotation + apply), bit for bit"""
    from castro_amd import _lib
    s, dt = _settings("all_vector"), DT
    geom = _lib.make_geom((32, 16, 16), prob_hi=(1.6, 0.8, 0.8))
    P = _lib.default_params()
    tabs, want = [], []
    for b in _stage_case():
        UO, M = _t(b["UO"]), [_t(m) for m in b["M"]]
        sb = (tuple(x - 3 for x in b["lo"]), tuple(x + 3 for x in b["hi"]))
        shape = (7,) + tuple(sb[1][a] - sb[0][a] + 1 for a in (2, 1, 0))
        Un, src = _t(b["UN"]), torch.zeros(shape, dtype=torch.float64, device="cuda")
        hydro.old_gravity_source(UO, b["gb"], src, sb, b["lo"], b["hi"], s["vec"], 4, dt)
        hydro.old_rotation_source(UO, b["gb"], src, sb, b["lo"], b["hi"], s["rot"], geom, dt)
        hydro.apply_source(Un, b["gb"], UO, b["gb"], dt, src, sb, 7, b["lo"], b["hi"], P, ntimes=1)
        want.append((Un, src))
        tabs.append((b, UO, _t(b["UN"]), torch.full(shape, 3.0, dtype=torch.float64, device="cuda"), sb, M, None, None))
    _one_pass(hydro, 0, tabs, s, geom, P, dt)
    torch.cuda.synchronize()
    for (Un, src), t in zip(want, tabs):
        v = _sl(t[0]["gb"], t[0]["lo"], t[0]["hi"])
        assert torch.equal(t[3], src) and torch.equal(t[2][v], Un[v])


def test_stage_2_refuses_diffusion_and_other_stages(hydro):
    from castro_amd import _lib
    b = _stage_case()[0]
    geom, P = _lib.make_geom((32, 16, 16), prob_hi=(1.6, 0.8, 0.8)), _lib.default_params()
    n = tuple(b["hi"][a] - b["lo"][a] + 1 for a in (2, 1, 0))
    UO, Un, src = _t(b["UO"]), _t(b["UN"]), torch.zeros((7,) + n, dtype=torch.float64, device="cuda")
    boxes = hydro.make_source_boxes([(b["lo"], b["hi"], (UO, b["gb"]), (Un, b["gb"]), (src, b["bx"]), [_t(m) for m in b["M"]], b["fb"])])
    keep = Un.clone()
    with pytest.raises(RuntimeError, match="unsupported option"):
        hydro.sources_mf(1 | _lib.SOURCES_AFTER_REFLUX, boxes, (0.0, 0.0, -1.0), 4, None, geom, P, DT, diffusion=_lib.make_diffusion(1.0))
    for stage in (2, 3, _lib.SOURCES_AFTER_REFLUX, 2 | _lib.SOURCES_AFTER_REFLUX):       # the flag goes with stage 1 only
        with pytest.raises(RuntimeError, match="bad argument"):
            hydro.sources_mf(stage, boxes, (0.0, 0.0, -1.0), 4, None, geom, P, DT)
    torch.cuda.synchronize()
    assert torch.equal(Un, keep)


# ---- 11. the driver -----------------------------------------------------------------------------------------------------------------
class _BoxByBox:
    """a HipHydro that shows neither the operation tables nor the level calls: CastroAmr goes box by box"""
    _hidden = ("make_ops", "fab_ops", "construct_ctu_hydro_source_mf")

    def __init__(self, h):
        self.__dict__["_h"] = h

    def __getattr__(self, name):
        if name in _BoxByBox._hidden:
            raise AttributeError(name)
        return getattr(self.__dict__["_h"], name)


def _reject(a, level, when):
    lev = a.lev[level]
    orig, n = lev.do_advance_ctu, [0]

    def do_advance_ctu(time, dt):
        n[0] += 1
        out = orig(time, dt)
        return (False, "forced rejection", None) if n[0] == when else out
    lev.do_advance_ctu = do_advance_ctu


def _scenario(name, make_hydro, params_of):
    """(hierarchy after its steps, dts): `gravity` -- test 2, one coarse step; `three levels` -- test 5, two coarse steps, gravity and
    rotation; `retry` -- test 6, the second fine advance rejected once"""
    kw = dict(do_grav=True, const_grav=-2.0)
    if name != "gravity":
        import castro_amd
        kw["rotation"] = castro_amd.make_rotation(2.0, rot_axis=3, center=(1.0, 0.5, 0.5))
    if name == "three levels":
        kw["patches"] = [R.FINE, R.FINER]
    a = R.make_amr(make_hydro, params_of(init_shrink=0.5), True, **kw)
    R.init_state(a)
    if name == "retry":
        _reject(a, 1, 2)
    dts = [a.step() for _ in range(2 if name == "three levels" else 1)]
    return a, dts


def _reference(oracle, name):
    if ("ref", name) not in _CACHE:
        a, dts = _scenario(name, R.RefluxOracleBackend, oracle.default_params)
        _CACHE[("ref", name)] = (dts, R.level_arrays(a), R.level_arrays(a, "new_source"),
                                 R.corrector_mismatch(a, 0, R.boundary_zones(a, 0)), [lev.nsubcycles for lev in a.lev])
    return _CACHE[("ref", name)]


@pytest.mark.parametrize("numerics", ["exact", "contract"])
@pytest.mark.parametrize("form", ["level calls", "tables", "box by box"])
@pytest.mark.parametrize("name", ["gravity", "three levels", "retry"])
def test_driver_on_the_device_against_the_oracle_backend(oracle, monkeypatch, name, form, numerics):
    """The option on the device in its three forms -- one stage-2 launch per level and one table launch per orientation (the
    default), the tables with the source stages box by box (CASTRO_AMD_LEVEL_CALLS=0), and every operation box by box (a
    backend without tables) -- against the oracle-backend run of the same scenario: dt sequence, S_new and new_source of every
    box of every level; `exact` bit for bit, `contract` within 1e-10 of a field's maximum.  The stored corrector passes the
    consistency bound of the CPU tests on the device too."""
    import castro_amd
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    monkeypatch.setenv("CASTRO_AMD_LEVEL_CALLS", "0" if form == "tables" else "1")

    def make_hydro():
        h = castro_amd.HipHydro(0, numerics=numerics)
        return _BoxByBox(h) if form == "box by box" else h
    want_dts, want_S, want_src, _, want_sub = _reference(oracle, name)
    a, dts = _scenario(name, make_hydro, castro_amd.default_params)
    torch.cuda.synchronize()
    assert [lev.batched for lev in a.lev[1:]] == [form != "box by box"] * (len(a.lev) - 1)
    assert (a.lev[0]._source_level_calls() is not None) == (form == "level calls")
    assert [lev.nsubcycles for lev in a.lev] == want_sub
    if numerics == "exact":
        assert dts == want_dts
    else:
        assert np.allclose(dts, want_dts, rtol=RTOL, atol=0.0)
    for which, want in (("S_new", want_S), ("new_source", want_src)):
        got = R.level_arrays(a, which)
        for l, (gl, wl) in enumerate(zip(got, want)):
            scale = np.max([np.abs(w).max(axis=(1, 2, 3)) for w in wl], axis=0)          # per field, over the level
            for g, w in zip(gl, wl):
                if numerics == "exact":
                    assert np.array_equal(g, w), "%s level %d: %d entries differ" % (which, l, int((g != w).sum()))
                else:
                    dev = np.abs(g - w).max(axis=(1, 2, 3)) / np.where(scale > 0, scale, 1.0)
                    assert dev.max() <= RTOL, (which, l, dev)
    assert R.corrector_mismatch(a, 0, R.boundary_zones(a, 0)) <= 1.e-11
