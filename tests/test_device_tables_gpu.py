"""GPU tests of the device tables behind the table-driven launches (castro_amd/csrc/dev_table.h; DESIGN.md "Device tables"):
the staged table of the source, diffusion, diagnostics, fab_ops and level-wide hydro launches, and the content-keyed cache of
the radial binning and of the point mass.

Every comparison is torch.equal against the same call on a fresh context: a table that was grown, reused at other offsets,
evicted and copied again, or found in the cache during a stream capture, changes no bit of what the kernels write."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from tests.util import physical_state

pytestmark = pytest.mark.gpu

_INPUTS = {}         # numpy inputs per (family, number of boxes)
_FRESH = {}          # outputs of a fresh context per (numerics, family, variant, number of boxes)


@pytest.fixture(scope="module", params=["exact", "contract"])
def numerics(request):
    if not torch.cuda.is_available():
        pytest.fail("the GPU tests need an MI355X")
    torch.cuda.set_device(0)
    return request.param


def _ctx(numerics):
    import castro_amd
    return castro_amd.HipHydro(0, numerics=numerics)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shape(box, ncomp):
    return (ncomp,) + tuple(box[1][a] - box[0][a] + 1 for a in (2, 1, 0))


def _grow(lo, hi, n):
    return tuple(x - n for x in lo), tuple(x + n for x in hi)


# ---- the inputs: boxes of 8^3 zones side by side in x, NUM_GROW ghost zones of state, 3 of source, 1 of gravity -------------------
def _box_inputs(nbox):
    if ("box", nbox) not in _INPUTS:
        rng = np.random.default_rng(100 + nbox)
        out = []
        for i in range(nbox):
            lo, hi = (8 * i, 8, 16), (8 * i + 7, 15, 23)
            gb, sb, vb = _grow(lo, hi, 4), _grow(lo, hi, 3), _grow(lo, hi, 1)
            fb, M = [], []
            for d in range(3):
                fhi = list(hi)
                fhi[d] += 1
                fb.append((lo, tuple(fhi)))
                M.append(rng.normal(size=_shape(fb[-1], 1)))
            UO, UN = physical_state(rng, gb[0], gb[1]), physical_state(rng, gb[0], gb[1])
            UO[6], UN[6] = rng.uniform(1.0, 2.0, size=UO[6].shape), rng.uniform(1.0, 2.0, size=UN[6].shape)     # a temperature to diffuse
            out.append(dict(lo=lo, hi=hi, gb=gb, sb=sb, vb=vb, fb=fb, M=M, UO=UO, UN=UN, src=rng.normal(size=_shape(sb, 7)),
                            gold=rng.uniform(-1.0, 1.0, size=_shape(vb, 3)), gnew=rng.uniform(-1.0, 1.0, size=_shape(vb, 3))))
        _INPUTS[("box", nbox)] = out
    return _INPUTS[("box", nbox)]


def _geom():
    from castro_amd import _lib
    return _lib.make_geom((48, 32, 32), prob_hi=(1.5, 1.0, 1.0))


def _source_specs(nbox):
    dev = [dict(b, UO=_t(b["UO"]), UN=_t(b["UN"]), src=_t(b["src"]), M=[_t(m) for m in b["M"]], gold=_t(b["gold"]), gnew=_t(b["gnew"]))
           for b in _box_inputs(nbox)]
    specs = [(b["lo"], b["hi"], (b["UO"], b["gb"]), (b["UN"], b["gb"]), (b["src"], b["sb"]), b["M"], b["fb"]) for b in dev]
    return dev, specs


def _run_sources(h, nbox, stage):
    from castro_amd import _lib
    dev, specs = _source_specs(nbox)
    h.sources_mf(stage, h.make_source_boxes(specs), (0.3, -0.7, -9.8), 4, None, _geom(), _lib.default_params(), 0.013, ntimes=1)
    return [b["src"] for b in dev] + [b["UN"] for b in dev]


def _run_sources_g(h, nbox, stage):
    from castro_amd import _lib
    dev, specs = _source_specs(nbox)
    h.sources_mf_g(stage, h.make_source_boxes(specs), h.make_grav_fabs([(b["gold"], b["vb"]) for b in dev]),
                   h.make_grav_fabs([(b["gnew"], b["vb"]) for b in dev]), 4, None, _geom(), _lib.default_params(), 0.013, ntimes=1)
    return [b["src"] for b in dev] + [b["UN"] for b in dev]


def _run_diffusion(h, nbox, _):
    from castro_amd import _lib
    dev, _specs = _source_specs(nbox)
    h.temp_diffusion_mf(h.make_diffusion_boxes([(b["lo"], b["hi"], (b["UO"], b["gb"]), (b["src"], b["sb"])) for b in dev]),
                        _lib.make_diffusion(3.0, 0.5, 1.0, 0.7), _geom(), 0.75)
    return [b["src"] for b in dev]


def _run_diag(h, nbox, _):
    from castro_amd import _lib
    dev, _specs = _source_specs(nbox)
    out = torch.full((_lib.DIAG_N,), 7.0, dtype=torch.float64, device="cuda")
    h.integrated_quantities_mf(h.make_diag_boxes([(b["lo"], b["hi"], (b["UO"], b["gb"]), None) for b in dev]), _geom(),
                               (0.7, 0.4, 0.6), out)
    return [out]


def _run_fab_ops(h, nops, _):
    """nops copies of 4^3 regions, two components, side by side in x; the regions beyond nops keep the fill"""
    from castro_amd import _lib
    if "ops" not in _INPUTS:
        _INPUTS["ops"] = np.random.default_rng(9).normal(size=(2, 4, 4, 4 * 48))
    box = ((0, 0, 0), (4 * 48 - 1, 3, 3))
    src, dst = _t(_INPUTS["ops"]), torch.full((2, 4, 4, 4 * 48), -1.0, dtype=torch.float64, device="cuda")
    ops = [(_lib.OP_COPY, 0, 2, (4 * r, 0, 0), (4 * r + 3, 3, 3), 0.0, 0.0, (dst, box), (src, box), None) for r in range(nops)]
    h.fab_ops(h.make_ops(ops), params=_lib.default_params())
    return [dst]


def _run_hydro_level(h, nbox, _):
    """boxes of 1 x 5 x 3 zones, the smallest of test_level_wide_launch_of_unequal_boxes_equals_the_per_box_calls; one box is the
    per-box call inside the library, two and more go through the table"""
    import castro_amd
    shape, dx = (1, 5, 3), (0.02, 0.015, 0.03)
    los = [(3 + 17 * n, 40 - 5 * n, 7 + 11 * n) for n in range(nbox)]
    his = [tuple(lo[d] + shape[d] - 1 for d in range(3)) for lo in los]
    if ("hydro", nbox) not in _INPUTS:
        rng = np.random.default_rng(300 + nbox)
        _INPUTS[("hydro", nbox)] = [physical_state(rng, *_grow(lo, hi, 4)) for lo, hi in zip(los, his)]
    G = castro_amd.make_geom((400, 400, 400), prob_hi=tuple(400 * d for d in dx))
    specs, outs = [], []
    for n, Unp in enumerate(_INPUTS[("hydro", nbox)]):
        lo, hi = los[n], his[n]
        U = _t(Unp)
        Sn = U[(slice(None),) + tuple(slice(4, 4 + shape[2 - a]) for a in range(3))].clone().contiguous()
        fl, mf, fb = [], [], []
        for d in range(3):
            fhi = list(hi)
            fhi[d] += 1
            fb.append((lo, tuple(fhi)))
            fl.append(h.alloc(8, lo, fhi))
            mf.append(h.alloc(1, lo, fhi))
        specs.append(((lo, hi), (lo, hi), (U, _grow(lo, hi, 4)), (Sn, (lo, hi)), fl, fb, mf))
        outs += [Sn] + fl + mf
    h.construct_ctu_hydro_source_mf(None, h.make_hydro_boxes(specs), G, castro_amd.default_params(), 0.0, 6.0e-4)
    torch.cuda.synchronize()
    assert h.status() == 0
    return outs


def _fresh(numerics, run, n, variant):
    key = (numerics, run.__name__, variant, n)
    if key not in _FRESH:
        h = _ctx(numerics)
        _FRESH[key] = run(h, n, variant)
        torch.cuda.synchronize()
        h.close()
    return _FRESH[key]


GROW_CASES = [("sources_mf stage 0", _run_sources, 0, (1, 5)), ("sources_mf stage 1", _run_sources, 1, (1, 5)),
              ("sources_mf_g stage 0", _run_sources_g, 0, (1, 5)), ("sources_mf_g stage 1", _run_sources_g, 1, (1, 5)),
              ("temp_diffusion_mf", _run_diffusion, None, (1, 5)), ("integrated_quantities_mf", _run_diag, None, (1, 5)),
              ("fab_ops", _run_fab_ops, None, (17, 48)),                       # 17: the first count that takes the table
              ("ctu_hydro_mf", _run_hydro_level, None, (1, 3)),
              ("ctu_hydro_mf through the table both times", _run_hydro_level, None, (2, 5))]


@pytest.mark.parametrize("name,run,variant,sizes", GROW_CASES, ids=[c[0].replace(" ", "_") for c in GROW_CASES])
def test_a_table_that_grew_and_is_reused_changes_no_bit(numerics, name, run, variant, sizes):
    """one context: a small table, one more than twice as large (the buffer is freed and allocated again), the small one again
    (the large buffer, the second part at another offset) -- each call gives the bits of a fresh context"""
    small, large = sizes
    h = _ctx(numerics)
    got = [run(h, n, variant) for n in (small, large, small)]
    torch.cuda.synchronize()
    h.close()
    for call, (g, n) in enumerate(zip(got, (small, large, small))):
        want = _fresh(numerics, run, n, variant)
        assert len(g) == len(want)
        for k, (a, b) in enumerate(zip(g, want)):
            assert not torch.isnan(b).any(), (name, "the reference holds NaN", n, k)
            assert torch.equal(a, b), "%s, call %d (%d entries), output %d: %d values differ" % (name, call, n, k, int((a != b).sum()))


# ---- the content-keyed cache ---------------------------------------------------------------------------------------------------
def _radial_setup():
    from castro_amd import _lib
    geom = _lib.make_geom((16, 16, 16))
    return geom, _lib.make_monopole((16, 16, 16), geom, (0.5, 0.5, 0.5), 2)


def _radial_states(n):
    if ("radial", n) not in _INPUTS:
        rng = np.random.default_rng(41)
        _INPUTS[("radial", n)] = [physical_state(rng, (4, 4, 4), (11, 11, 11)) for _ in range(n)]
    return [_t(u) for u in _INPUTS[("radial", n)]]


def test_radial_mass_after_its_table_was_evicted(numerics):
    """nine single-box tables of 8^3 zones on one context (the cache of the binning keeps eight), then the first again: the
    bits of a fresh context"""
    geom, mono = _radial_setup()
    box = ((4, 4, 4), (11, 11, 11))
    states = _radial_states(9)
    h = _ctx(numerics)
    outs = []
    for U in states + states[:1]:
        outs.append(torch.full((2 * mono.n1d,), float("nan"), dtype=torch.float64, device="cuda"))
        h.radial_mass_mf(h.make_diag_boxes([(box[0], box[1], (U, box), None)]), geom, mono, outs[-1])
    torch.cuda.synchronize()
    h.close()
    f = _ctx(numerics)
    for k in (0, 8):
        want = torch.full((2 * mono.n1d,), float("nan"), dtype=torch.float64, device="cuda")
        f.radial_mass_mf(f.make_diag_boxes([(box[0], box[1], (states[k], box), None)]), geom, mono, want)
        torch.cuda.synchronize()
        assert not torch.isnan(want).any() and float(want[:mono.n1d].sum()) > 0.0
        assert torch.equal(outs[k], want), k
        if k == 0:
            assert torch.equal(outs[9], want), "the first table again"
    f.close()


def test_add_pointmass_after_its_table_was_evicted(numerics):
    """33 tables of one 4^3 gravity FAB on one context (the cache of the point mass keeps 32), then the first again: the FAB
    that took the field twice holds the bits of two calls on a fresh context"""
    from castro_amd import _lib
    geom, pm = _lib.make_geom((16, 16, 16)), _lib.make_pointmass((0.5, 0.5, 0.5))
    box = ((2, 3, 4), (5, 6, 7))
    mass = torch.full((1,), 2.5e30, dtype=torch.float64, device="cuda")
    base = _t(np.random.default_rng(3).normal(size=(3, 4, 4, 4)))
    fabs = [base.clone() for _ in range(33)]
    h = _ctx(numerics)
    for g in fabs + fabs[:1]:
        h.add_pointmass_mf(h.make_grav_fabs([(g, box)]), pm, geom, mass)
    torch.cuda.synchronize()
    h.close()
    f = _ctx(numerics)
    once, twice = base.clone(), base.clone()
    f.add_pointmass_mf(f.make_grav_fabs([(once, box)]), pm, geom, mass)
    for _ in range(2):
        f.add_pointmass_mf(f.make_grav_fabs([(twice, box)]), pm, geom, mass)
    torch.cuda.synchronize()
    f.close()
    assert not torch.equal(once, base) and not torch.equal(twice, once)
    assert torch.equal(fabs[0], twice), "the first table again"
    for k in range(1, 33):
        assert torch.equal(fabs[k], once), k


def _capture(fn):
    """fn captured on one stream (a linear graph); no finaliser frees device memory inside the capture"""
    gc.collect()
    gc.disable()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
    finally:
        gc.enable()
    torch.cuda.synchronize()
    return g


def test_a_radial_mass_call_that_hits_the_cache_can_be_captured(numerics):
    """DESIGN.md "Device tables": a call whose table the context has seen neither allocates nor synchronises"""
    geom, mono = _radial_setup()
    box = ((4, 4, 4), (11, 11, 11))
    U = _radial_states(9)[0]
    h = _ctx(numerics)
    table = h.make_diag_boxes([(box[0], box[1], (U, box), None)])
    eager = torch.full((2 * mono.n1d,), float("nan"), dtype=torch.float64, device="cuda")
    h.radial_mass_mf(table, geom, mono, eager)
    torch.cuda.synchronize()
    out = torch.zeros(2 * mono.n1d, dtype=torch.float64, device="cuda")
    g = _capture(lambda: h.radial_mass_mf(table, geom, mono, out))
    assert float(out.abs().sum()) == 0.0, "captured, not executed"
    g.replay()
    torch.cuda.synchronize()
    assert float(eager[:mono.n1d].sum()) > 0.0 and torch.equal(out, eager)
    del g
    h.close()


def test_a_pointmass_update_that_hits_the_cache_can_be_captured(numerics):
    """pointmass_delta_mf + pointmass_apply_mf of one 8^3 box around the centre, mass arriving in the cube: eager once, then
    the same pair captured and replayed on the restored arrays"""
    from castro_amd import _lib
    geom, pm = _lib.make_geom((16, 16, 16)), _lib.make_pointmass((0.5, 0.5, 0.5))
    box = ((4, 4, 4), (11, 11, 11))
    rng = np.random.default_rng(17)
    So = _t(physical_state(rng, *box))
    new0 = So.clone()
    new0[0] *= 1.25                                                               # rho grew everywhere: delta > 0
    Sn, mass, delta = new0.clone(), torch.full((1,), 3.0, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    h = _ctx(numerics)
    boxes = h.make_pointmass_boxes([(box[0], box[1], (So, box), (Sn, box))])

    def pair():
        h.pointmass_delta_mf(boxes, pm, geom, delta)
        h.pointmass_apply_mf(boxes, pm, geom, delta, mass)

    pair()
    torch.cuda.synchronize()
    eager = (Sn.clone(), mass.clone(), delta.clone())
    assert float(eager[2]) > 0.0 and float(eager[1]) == 3.0 + float(eager[2]) and not torch.equal(eager[0], new0)
    Sn.copy_(new0); mass.fill_(3.0); delta.zero_()
    torch.cuda.synchronize()
    g = _capture(pair)
    assert torch.equal(Sn, new0) and float(mass) == 3.0, "captured, not executed"
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(Sn, eager[0]) and torch.equal(mass, eager[1]) and torch.equal(delta, eager[2])
    del g
    h.close()


# ---- the refusals of the one-pass source entry points ---------------------------------------------------------------------------
REFUSALS = [(entry, case) for entry in ("sources_mf", "sources_mf_ex", "sources_mf_g", "sources_mf_opts", "sources_mf_opts with gravity FABs")
            for case in ("no boxes", "bad stage", "small mass flux")] + [("sources_mf_opts with gravity FABs", "diffusion")]


@pytest.mark.parametrize("entry,case", REFUSALS, ids=["%s-%s" % (e.replace(" ", "_"), c.replace(" ", "_")) for e, c in REFUSALS])
def test_refusals_of_the_source_entry_points(numerics, entry, case):
    """the code each public entry point returns for: an empty level (accepted), a stage that is neither 0 nor 1, a mass-flux
    FAB one face short in stage 1, gravity FABs together with diffusion"""
    from castro_amd import _lib
    want = {"no boxes": _lib.OK, "bad stage": _lib.ERR_ARG, "small mass flux": _lib.ERR_ARG, "diffusion": _lib.ERR_UNSUPPORTED}[case]
    h = _ctx(numerics)
    dev, specs = _source_specs(1)
    b = dev[0]
    if case == "small mass flux":
        specs[0][5][1] = specs[0][5][1][:, :, :-1, :].contiguous()                # the y faces: hi[1] + 1 is missing
        fb = list(specs[0][6])
        fb[1] = (b["lo"], b["hi"])
        specs[0] = specs[0][:6] + (fb,)
    arr, n = h.make_source_boxes(specs)
    n = 0 if case == "no boxes" else n
    stage = 2 if case == "bad stage" else 1
    before = [b["src"].clone(), b["UN"].clone()]
    geom, P, diff = _geom(), _lib.default_params(), _lib.make_diffusion(3.0)
    vec = (C.c_double * 3)(0.3, -0.7, -9.8)
    go, gn = h.make_grav_fabs([(b["gold"], b["vb"])]), h.make_grav_fabs([(b["gnew"], b["vb"])])
    tail = (C.byref(geom), C.byref(P), 0.013, 1, None)
    if entry == "sources_mf":
        rc = h.lib.castro_amd_sources_mf(h.h, stage, n, arr, vec, 4, None, *tail)
    elif entry == "sources_mf_ex":
        rc = h.lib.castro_amd_sources_mf_ex(h.h, stage, n, arr, vec, 4, None, C.byref(diff), *tail)
    elif entry == "sources_mf_g":
        rc = h.lib.castro_amd_sources_mf_g(h.h, stage, n, arr, go, gn, 4, None, *tail)
    else:
        if entry.endswith("gravity FABs"):
            opts = _lib.SourceOpts(None, go, gn, 4)
            if case == "diffusion":
                opts.diff = C.pointer(diff)
        else:
            opts = _lib.SourceOpts(C.cast(vec, C.POINTER(C.c_double)), None, None, 4)
        rc = h.lib.castro_amd_sources_mf_opts(h.h, stage, n, arr, C.byref(opts), *tail)
    torch.cuda.synchronize()
    h.close()
    assert rc == want, (entry, case, rc)
    assert torch.equal(b["src"], before[0]) and torch.equal(b["UN"], before[1]), "a refused or empty call writes nothing"
