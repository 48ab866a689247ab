"""Robust normalisation without a GPU: the numpy statement of include/microaligner_quantile.h (tests/_quantile_ref.py) against
np.quantile(method="lower") and against the oracle's min-max normalisation, what percentile scaling buys on an image with one
hot pixel, the parameter checks, the MA_EINVAL paths of the two C entries, the build wiring and the CLI schema."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _quantile_ref as R  # noqa: E402
from microaligner_amd import pipeline as P  # noqa: E402
from microaligner_amd.device import QuantileCounts, image_quantiles_params, normalize_range_params  # noqa: E402
from microaligner_amd.shared_modules.normalize import NormalizeInfo, percentile_params, percentile_ranks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_quantile.h")
QS = (0.0, 0.001, 0.25, 0.5, 0.999, 1.0)


def arrays_4097():
    rng = np.random.default_rng(11)
    return {"u8": rng.integers(0, 256, 4097, dtype=np.uint8),
            "u16": rng.integers(0, 65536, 4097).astype(np.uint16),
            "f32": (rng.standard_normal(4097) * 1e3).astype(np.float32)}


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_statement_is_numpy_quantile_lower(kind):
    a = arrays_4097()[kind]
    vals, (pop, nonfinite, zeros) = R.image_quantiles(a, QS)
    assert (pop, nonfinite, zeros) == (4097, 0, 0) and vals.dtype == np.float64
    for q, v in zip(QS, vals):
        assert v == float(np.quantile(a, q, method="lower")), q
    assert vals[0] == float(a.min()) and vals[-1] == float(a.max())
    # the population rules: non-finite values and, on request, zeros are left out and counted; -0.0 is +0.0
    if kind == "f32":
        b = a.copy()
        b[::7] = np.nan
        b[3::11] = np.inf
        b[5::13] = -np.inf
        b[1::17] = -0.0
        fin = b[np.isfinite(b)]
        vals, counts = R.image_quantiles(b, QS)
        assert counts == (fin.size, b.size - fin.size, 0)
        assert np.array_equal(vals, [float(np.quantile(fin, q, method="lower")) for q in QS])
        vals, counts = R.image_quantiles(b, [0.5], ignore_zeros=True)
        nz = fin[fin != 0]
        assert counts == (nz.size, b.size - fin.size, fin.size - nz.size) and vals[0] == float(np.quantile(nz, 0.5, method="lower"))
        z = R.image_quantiles(np.array([-0.0, 0.0, -0.0], np.float32), [0.0, 1.0])[0]
        assert not np.signbit(z).any()
    assert np.isnan(R.image_quantiles(np.zeros(5, a.dtype), [0.0, 1.0], ignore_zeros=True)[0]).all()


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_range_statement_at_min_max_is_the_oracles_minmax_normalisation(kind):
    from oracle import oracle as O
    a = arrays_4097()[kind].reshape(17, 241)
    assert np.array_equal(R.normalize_range_u8(a, float(a.min()), float(a.max())), O.normalize_minmax_u8(a.astype(np.float32)))
    c = np.full((5, 7), a.flat[0], a.dtype)                                   # a constant image: all zeros
    assert not R.normalize_range_u8(c, float(c.min()), float(c.max())).any() and not O.normalize_minmax_u8(c.astype(np.float32)).any()
    special = np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0, 10.0, 5.0, 4.999, 10.0001], np.float32)
    assert R.normalize_range_u8(special, 0.0, 10.0).tolist() == [0, 255, 0, 255, 0, 0, 255, 128, 127, 255]
    assert not R.normalize_range_u8(special, 3.0, 3.0).any() and not R.normalize_range_u8(special, 3.0, 2.0).any()


def test_one_hot_pixel_costs_min_max_scaling_its_grey_levels():
    """The case the feature is for: 301 x 517 uint16, background 200 + Poisson(30), nuclei up to ~2700, one pixel at 65535."""
    img = R.hot_pixel_image()
    assert img.shape == (301, 517) and img.dtype == np.uint16 and int((img == 65535).sum()) == 1
    minmax = R.normalize_range_u8(img, float(img.min()), float(img.max()))
    robust, info = R.normalize_percentile(img, 0.0, 99.9)
    print("grey levels: min-max", len(np.unique(minmax)), "percentile (0, 99.9)", len(np.unique(robust)), info)
    assert len(np.unique(minmax)) < 16
    assert len(np.unique(robust)) > 128
    assert not info["degenerate"] and info["lo"] == float(img.min()) and info["hi"] < 3000
    assert float((img > info["hi"]).mean()) <= 0.001 + 1.0 / img.size


def test_parameter_checks_need_no_device():
    a = np.zeros((3, 4), np.uint16)
    dt, n, qs, flags = image_quantiles_params(a, [0.5, 0.0, 0.5])
    assert (dt, n, flags) == (1, 12, 0) and qs.dtype == np.float64 and qs.tolist() == [0.5, 0.0, 0.5]
    assert image_quantiles_params(a, 1.0, ignore_zeros=True)[2:] [0].tolist() == [1.0]
    assert image_quantiles_params(a, 1.0, ignore_zeros=True)[3] == 1
    for bad in (dict(q=[]), dict(q=[0.1] * 9), dict(q=[-0.1]), dict(q=[1.0001]), dict(q=[float("nan")]), dict(q="x"),
                dict(q=[[0.1, 0.2]]), dict(q=[0.5], ignore_zeros=1)):
        with pytest.raises(ValueError):
            image_quantiles_params(a, **bad)
    for arr in (np.zeros((3, 4), np.float64), np.zeros((0, 4), np.uint8), [1, 2, 3]):
        with pytest.raises(ValueError):
            image_quantiles_params(arr, [0.5])
        with pytest.raises(ValueError):
            normalize_range_params(arr, 0.0, 1.0)
    assert normalize_range_params(a, 1, 2.5) == (1, 12, 1.0, 2.5)
    for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), ("0", 1.0), (True, 2.0)):
        with pytest.raises(ValueError):
            normalize_range_params(a, lo, hi)
    assert percentile_params(0, 99.9) == (0.0, 99.9 / 100.0) and percentile_params(np.float32(50), 100) == (0.5, 1.0)
    for low, high in ((50, 50), (60, 40), (-1, 50), (0, 100.5), (float("nan"), 50), (0, float("nan")), ("0", 50), (False, 50)):
        with pytest.raises(ValueError):
            percentile_params(low, high)
    with pytest.raises(ValueError):
        percentile_params(0, 50, ignore_zeros="yes")
    assert percentile_ranks(0, 99.9, 155617) == (0, int(np.floor(0.999 * 155616.0)))
    assert QuantileCounts(1, 2, 3).zeros == 3 and NormalizeInfo._fields == ("lo", "hi", "pop", "nonfinite", "zeros", "degenerate")
    # the wrappers check before any device work
    import microaligner_amd
    from microaligner_amd.shared_modules import utils
    with pytest.raises(ValueError):
        microaligner_amd.normalize_percentile(a, 50, 50)
    with pytest.raises(ValueError):
        utils.max_project_and_normalize(a[None], percentiles=(0, 101))
    with pytest.raises(ValueError):
        utils.max_project_and_normalize(a[None], percentiles=(5,))
    with pytest.raises(ValueError):
        utils.max_project_and_normalize(a[None], ignore_zeros=True)
    assert {"normalize_percentile", "NormalizeInfo"} <= set(microaligner_amd.__all__)


def test_c_entries_reject_bad_arguments_without_a_device():
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    p = C.c_void_p(0x1000)            # never dereferenced: every call below fails its checks
    q = (C.c_double * 9)(0.0, 0.5, 1.0, 0.25, 0.75, 0.1, 0.9, 0.99, 0.01)
    vals, counts = (C.c_double * 9)(), (C.c_longlong * 3)()

    def quant(ctx=p, img=p, dtype=_lib.MA_U16, n=100, flags=0, q=q, nq=2, values=vals, counts=counts):
        return lib.ma_image_quantiles(ctx, img, dtype, n, flags, q, nq, values, counts)

    def rng(ctx=p, src=p, dtype=_lib.MA_U16, n=100, lo=0.0, hi=1.0, dst=p):
        return lib.ma_normalize_range_u8(ctx, src, dtype, n, lo, hi, dst)

    for kw in (dict(ctx=None), dict(img=None), dict(q=None), dict(values=None), dict(counts=None)):
        assert quant(**kw) == _lib.MA_EINVAL, kw
        assert b"NULL" in lib.ma_last_error()
    for kw in (dict(n=0), dict(n=(1 << 40) + 1), dict(dtype=3), dict(dtype=-1), dict(nq=0), dict(nq=9), dict(flags=2), dict(flags=-1),
               dict(q=(C.c_double * 2)(0.5, float("nan"))), dict(q=(C.c_double * 2)(-1e-9, 0.5)), dict(q=(C.c_double * 2)(0.5, 1.0000001))):
        assert quant(**kw) == _lib.MA_EINVAL, kw
        assert b"invalid argument" in lib.ma_last_error()
    for kw in (dict(ctx=None), dict(src=None), dict(dst=None)):
        assert rng(**kw) == _lib.MA_EINVAL and b"NULL" in lib.ma_last_error(), kw
    for kw in (dict(n=0), dict(dtype=7), dict(lo=float("nan")), dict(hi=float("inf")), dict(lo=float("-inf"))):
        assert rng(**kw) == _lib.MA_EINVAL, kw


def test_header_bindings_and_build_wiring_agree(monkeypatch):
    from microaligner_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_image_quantiles", "ma_normalize_range_u8"] == sorted(_lib.QUANTILE_SIGNATURES)
    for n in names:
        proto = re.search(r"\b" + n + r"\s*\((.*?)\)\s*;", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.QUANTILE_SIGNATURES[n][1]), n
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES") and k != "QUANTILE_SIGNATURES"]
    assert len(others) >= 15 and not any(set(_lib.QUANTILE_SIGNATURES) & set(t) for t in others)
    defs = {k: v for k, v in re.findall(r"#define\s+(MA_Q_[A-Z_]+)\s+(.+)", text)}
    assert int(defs["MA_Q_IGNORE_ZEROS"]) == _lib.MA_Q_IGNORE_ZEROS and int(defs["MA_Q_MAX_RANKS"]) == _lib.MA_Q_MAX_RANKS
    assert defs["MA_Q_MAX_PIXELS"].strip() == "(1LL << 40)" and _lib.MA_Q_MAX_PIXELS == 1 << 40
    build.build()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    # quantile.hip is built, is off the measured path, and is rebuilt when its header changes
    assert "quantile.hip" in build.SOURCES
    assert [os.path.abspath(h) for h in build.SOURCE_HEADERS["quantile.hip"]] == [HEADER]
    assert build.source_hash() == _lib.source_hash()
    before = build.source_hash()
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "quantile.hip"])
    assert build.source_hash() == before, "quantile.hip must not enter the hash of the measured path"
    # the kernels keep to d_cvround / d_clamp of ma_internal.h and leave dog.hip's scale_to_u8 alone
    src = open(os.path.join(build.CSRC, "quantile.hip")).read()
    assert "d_cvround" in src and "d_clamp" in src and "scale_to_u8" not in src and "__builtin_nontemporal_store" in src


REG = dict(NumberPyramidLevels=2, NumberIterationsPerLevel=3, TileSize=150, Overlap=30, NumberOfWorkers=0,
           UseFullResImage=True, UseDOG=False)


def _cfg(section, **keys):
    return {"Input": {"InputImagePaths": {"Cycle 1": "a.npy", "Cycle 2": "b.npy"}, "ReferenceCycle": 1, "ReferenceChannel": "0"},
            "Output": {"OutputDir": "out", "OutputPrefix": "x_", "SaveOutputToCycleStack": True},
            "RegistrationParameters": {section: dict(REG, **keys)}}


@pytest.mark.parametrize("section", ["FeatureReg", "OptFlowReg"])
def test_cli_schema_takes_the_two_keys_under_both_sections(section):
    attr = "feature" if section == "FeatureReg" else "optflow"
    plain = getattr(P.PipelineConfig(_cfg(section)), attr)
    assert plain.NormalizePercentiles is None and plain.NormalizeIgnoreZeros is False
    got = getattr(P.PipelineConfig(_cfg(section, NormalizePercentiles=[0, 99.9], NormalizeIgnoreZeros=True)), attr)
    assert got.NormalizePercentiles == (0.0, 99.9) and got.NormalizeIgnoreZeros is True
    assert getattr(P.PipelineConfig(_cfg(section, NormalizePercentiles=[1.5, 100])), attr).NormalizePercentiles == (1.5, 100.0)
    # the registrators' own keyword sets are what they were
    assert "NormalizePercentiles" not in got.feature_kwargs() and "normalize_percentiles" not in got.optflow_kwargs()
    for bad in ([99.9], [0, 50, 99], [50, 50], [60, 40], [-1, 50], [0, 100.5], ["0", 99], [0, True], (0, 99.9), 99.9, "0,99"):
        with pytest.raises((TypeError, ValueError), match="NormalizePercentiles"):
            P.PipelineConfig(_cfg(section, NormalizePercentiles=bad))
    for bad in ("yes", 1, None, [True]):
        with pytest.raises((TypeError, ValueError), match="NormalizeIgnoreZeros"):
            P.PipelineConfig(_cfg(section, NormalizePercentiles=[0, 99.9], NormalizeIgnoreZeros=bad))
    with pytest.raises(ValueError, match="needs NormalizePercentiles"):
        P.PipelineConfig(_cfg(section, NormalizeIgnoreZeros=True))


def test_cycle_chain_takes_the_options_out_of_its_params(monkeypatch):
    """parallel.register_cycle_chain: normalize_percentiles / normalize_ignore_zeros reach max_project_and_normalize and not
    the registrator."""
    from microaligner_amd import parallel
    from microaligner_amd.shared_modules import utils
    seen = []

    class Stop(Exception):
        pass

    def fake(pages, **kw):
        seen.append(kw)
        raise Stop

    monkeypatch.setattr(utils, "max_project_and_normalize", fake)
    cycles = [np.zeros((1, 1, 4, 4), np.uint8)] * 2
    with pytest.raises(Stop):
        parallel.register_cycle_chain(cycles, params=dict(tile_size=150, normalize_percentiles=(1, 99), normalize_ignore_zeros=True))
    with pytest.raises(Stop):
        parallel.register_cycle_chain(cycles, params=dict(tile_size=150))
    assert seen == [dict(on_device=True, percentiles=(1, 99), ignore_zeros=True), dict(on_device=True)]
    with pytest.raises(ValueError, match="normalize_percentiles"):
        parallel.register_cycle_chain(cycles, params=dict(normalize_ignore_zeros=True))
