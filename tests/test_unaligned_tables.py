"""The tables of tests/test_gpu_unaligned.py without a GPU: the offsets of the shifted allocator, and that every entry and
parameter the rejection and override tables name is one of the headers and of the bindings, and that the tables account for
every alignment check of the sources."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases  # noqa: E402  (the registry: declared_entries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prototypes():
    """entry -> the parameter names of its prototype, from every header under include/ (comments stripped, as
    tests/test_abi.py reads them)"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        for name, params in re.findall(r"\bint\s+(ma_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d*\])?\s*$", p.strip()).group(1) for p in params.split(",")]
            assert name not in out, name
            out[name] = names
    return out


def bindings():
    from microaligner_amd import _lib
    return {name: sig for n, d in vars(_lib).items() if n.endswith("SIGNATURES") and isinstance(d, dict) for name, sig in d.items()}


DTYPES = (np.uint8, np.uint16, np.int32, np.float32, np.int64, np.float64)


def test_offsets_have_the_residues_of_the_two_passes():
    import test_gpu_unaligned as U
    for dtype in DTYPES:
        size = np.dtype(dtype).itemsize
        for shape in ((5,), (3, 7), (2,), (4, 5, 3)):
            assert U.alignment_of(shape, dtype) == size
            assert U.offset_for(shape, dtype, "edge") % 16 == size          # A (mod 16): off every larger boundary
            assert U.offset_for(shape, dtype, "half") % 16 == 8 and U.offset_for(shape, dtype, "half") % size == 0
        for shape in ((7, 2), (3, 5, 2)):
            a = 2 * size
            assert U.alignment_of(shape, dtype) == a
            edge, half = U.offset_for(shape, dtype, "edge"), U.offset_for(shape, dtype, "half")
            if a <= 8:
                assert edge % 16 == a and half % 16 == 8
            else:
                assert a == 16 and edge % 32 == 16 and half == edge
    for off in [U.offset_for(s, d, w) for d in DTYPES for s in ((5,), (7, 2)) for w in U.PASSES]:
        assert 0 < off < U.SLACK
    with pytest.raises(AssertionError):
        U.offset_for((5,), np.float32, "neither")


def test_overrides_raise_the_alignment_of_their_kind_only():
    import test_gpu_unaligned as U
    f64, pair = {"f64": 32}, {"pair": 16}
    for which in U.PASSES:
        assert U.offset_for((130, 4), np.float64, which, f64) % 64 == 32        # cw
        assert U.offset_for((400, 2), np.float64, which, f64) % 64 == 32        # points
        assert U.offset_for((40, 50, 2), np.float32, which, pair) % 32 == 16    # a flow
    assert U.offset_for((37, 515, 2), np.float32, "edge", f64) % 16 == 8        # the flow of the landmark case: the rule's
    assert U.offset_for((79, 99), np.float32, "edge", pair) % 16 == 4           # an image of a pair case: the rule's
    assert U.raw_alignment() == 16 and U.raw_alignment(f64) == 32 and U.raw_alignment(pair) == 16
    for name, (override, sentence) in U.OVERRIDES.items():
        assert set(override) <= {"f64", "pair"} and all(v in (16, 32) for v in override.values()), name
        # the sentence it quotes stands in the header it names
        header, quoted = re.match(r"(include/\w+\.h)[^\"]*\"(.*)\"$", sentence).groups()
        text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, header)).read())
        assert quoted in text, (name, quoted)


def test_every_rejected_parameter_is_one_of_the_headers_and_of_the_bindings():
    import test_gpu_unaligned as U
    protos, sigs = prototypes(), bindings()
    assert len(protos) > 100
    seen = set()
    for entry, param, nbytes, pos in U.REJECT:
        assert (entry, param) not in seen, (entry, param)
        seen.add((entry, param))
        assert entry in protos and entry in sigs, entry
        assert protos[entry][0] == "ctx" and protos[entry][pos] == param, (entry, param, protos[entry])
        assert sigs[entry][1][pos] is C.c_void_p, (entry, param)
        assert nbytes in (8, 16, 32)
        assert entry in U.CALLS and entry in _gpu_cases.declared_entries(), entry
    assert set(U.CALLS) == {e for e, _, _, _ in U.REJECT}
    # the valid calls have the arguments of the prototypes, each of a type its ctypes prototype converts
    from types import SimpleNamespace as NS
    from microaligner_amd import _lib as L
    b = NS(p=[(k + 1) << 16 for k in range(6)], m6=(C.c_double * 6)(), taps=(C.c_float * 2)(), pages=(C.c_void_p * 1)(),
           outs=(C.c_void_p * 1)(), d=(C.c_double * 16)(), d2=(C.c_double * 16)(), d3=(C.c_double * 16)(),
           ll=(C.c_longlong * 16)(), ll2=(C.c_longlong * 16)(), f=(C.c_float * 16)(), ref=NS(ptr=7 << 16), mov=NS(ptr=8 << 16),
           reg_flow=NS(ptr=9 << 16), params=L.MaParams(), reports=(L.MaLevelReport * 4)(), n_reports=C.c_int(0))
    for entry, call in U.CALLS.items():
        args, types = call(b), sigs[entry][1][1:]
        assert len(args) == len(types) == len(protos[entry]) - 1, (entry, len(args), len(types))
        for k, (a, t) in enumerate(zip(args, types)):
            t.from_param(a)                                          # TypeError / ArgumentError if it does not fit
            if t in (C.c_int, C.c_size_t):
                assert isinstance(a, int) and abs(a) < 1 << 16, (entry, k, a)      # a size, not an address
    for entry, param, nbytes, pos in U.REJECT:
        a = U.CALLS[entry](b)[pos - 1]
        assert isinstance(a, int) and a % 64 == 0 and a >= 1 << 16, (entry, param)
    # the valid call of BELOW likewise: ma_normalize_local, each moved parameter at the position of its name in the prototype
    entry = "ma_normalize_local"
    assert entry in protos and entry in sigs and entry in _gpu_cases.declared_entries() and entry not in U.CALLS
    assert len(set(U.BELOW)) == len(U.BELOW)
    for param, dtype, kind, nbytes, by in U.BELOW:
        good = U.below_call(b.p[:4], dtype, kind, b.taps, (C.c_longlong * 4)())
        args, types = list(good.values()), sigs[entry][1][1:]
        assert len(args) == len(types) == len(protos[entry]) - 1
        for k, (a, t) in enumerate(zip(args, types)):
            t.from_param(a)
            if t is C.c_int:
                assert isinstance(a, int) and abs(a) < 1 << 16, (entry, k, a)
        pos = 1 + list(good).index(param)
        assert protos[entry][0] == "ctx" and protos[entry][pos] == param and sigs[entry][1][pos] is C.c_void_p, (param, pos)
        assert isinstance(good[param], int) and good[param] % 64 == 0 and good[param] >= 1 << 16, param
        # the element at that pointer in this call has nbytes bytes, and the pointer moved by `by` is not a multiple of it
        element = {"img": {L.MA_U8: 1, L.MA_U16: 2, L.MA_F32: 4}[dtype], "weight": 4 if kind == L.MA_SMOOTH_WEIGHT_F32 else 1,
                   "out_f32": 4}[param]
        assert nbytes == element and 0 < by < nbytes


def test_every_checked_parameter_of_the_sources_is_in_the_rejection_table():
    """every MA_REQUIRE_ALIGNED(ptr, size, "name") in an entry of csrc/ is accounted for: with a literal size <-> a row of
    REJECT; with any other size <-> a row of ELEMENT_SIZED, whose parameters are those of BELOW.  Nothing checked is left
    untested, and the tables name nothing the sources do not check"""
    import test_gpu_unaligned as U
    csrc = os.path.join(ROOT, "microaligner_amd", "csrc")
    uses, literal, found, sized = 0, 0, set(), []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        text = open(path).read()
        uses += len(re.findall(r"MA_REQUIRE_ALIGNED\s*\(", text))
        for m in re.finditer(r"MA_REQUIRE_ALIGNED\((\w+), ([^;\n]+?), \"(\w+)\"\)", text):
            assert m.group(1) == m.group(3), (path, m.group(0))
            if re.fullmatch(r"\d+", m.group(2)):
                literal += 1
                found.add((os.path.basename(path), m.group(3), int(m.group(2))))
            else:
                sized.append((os.path.basename(path), m.group(3), m.group(2)))
    table = {(p, n) for _, p, n, _ in U.REJECT}
    assert {(p, n) for _, p, n in found} == table, ({(p, n) for _, p, n in found} ^ table)
    assert sorted(sized) == sorted(U.ELEMENT_SIZED), (sized, U.ELEMENT_SIZED)
    assert {p for _, p, _ in U.ELEMENT_SIZED} == {p for p, _, _, _, _ in U.BELOW}
    # BELOW moves each of them, at every element size above one byte that it can have, by an odd number of bytes and by an
    # even one that is no multiple of the element
    sizes = {"img": (2, 4), "weight": (4,), "out_f32": (4,)}
    assert sorted((p, n, by) for p, _, _, n, by in U.BELOW) == sorted((p, n, by) for p, ns in sizes.items() for n in ns
                                                                      for by in (1, 2) if by < n)
    assert literal + len(sized) == uses, (literal, len(sized), uses)       # no use that neither pattern reads
    helper = open(os.path.join(csrc, "ma_internal.h")).read()
    assert "#define MA_REQUIRE_ALIGNED(ptr, bytes, name)" in helper and "must be %d-byte aligned" in helper
    # no hand-written alignment refusal is left beside the helper
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        assert not re.search(r"MA_REQUIRE\([^;]*byte aligned", open(path).read()), path


def test_the_rule_is_written_once_and_referenced():
    main = open(os.path.join(ROOT, "include", "microaligner_hip.h")).read()
    assert main.count("Device pointers (the alignment rule") == 1
    for word in ("aligned to its element", "8 bytes for pairs of float32", "16 bytes for pairs of float64", "MA_EINVAL"):
        assert word in main[main.index("Device pointers (the alignment rule"):][:1500], word
    up = main[main.index("cv2.pyrUp(flow * scale"):main.index("int ma_pyr_up_flow")]
    assert "dst must be 16-byte aligned" in up
    for name in ("compose", "flowcompose", "flowgrid", "flowinvert", "flowsmooth", "interp", "landmarks", "qc", "flowmedian",
                 "flowfill", "flowrefine", "flowaffine"):
        assert 'alignment rule of microaligner_hip.h ("Device pointers")' in open(
            os.path.join(ROOT, "include", f"microaligner_{name}.h")).read(), name
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        assert '"Device pointers"' in open(os.path.join(ROOT, doc)).read(), doc
