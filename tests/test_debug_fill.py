"""The test hook that fills a context's idle scratch memory (include/microaligner_debug.h, csrc/debug_fill.hip) and the
registry of GPU cases (tests/_gpu_cases) that tests/test_gpu_stale_memory.py runs with it.  CPU: the header <-> library <->
bindings agreement, the measured path's source hash, refused arguments that need no device, and the completeness of the
registry -- every C entry of the bindings is either exercised by a case on stale scratch memory or named in EXEMPT, which
may only hold entries that launch no kernel over scratch memory."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases as S  # noqa: E402  (the registry: CASES, EXEMPT, declared_entries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_debug.h")


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))


def test_debug_header_library_and_bindings_agree():
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert _declared(HEADER) == ["ma_debug_fill_idle"]
    assert hasattr(lib, "ma_debug_fill_idle"), "declared in microaligner_debug.h but not exported"
    assert sorted(_lib.DEBUG_SIGNATURES) == ["ma_debug_fill_idle"], "ctypes prototypes out of sync with microaligner_debug.h"
    others = [d for n, d in vars(_lib).items() if n.endswith("SIGNATURES") and n != "DEBUG_SIGNATURES"]
    assert others and not any(set(_lib.DEBUG_SIGNATURES) & set(d) for d in others)
    assert '#include "microaligner_hip.h"' in open(HEADER).read()
    res, args = _lib.DEBUG_SIGNATURES["ma_debug_fill_idle"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
    # the hook is a method of the context and not part of the package's interface
    import microaligner_amd
    from microaligner_amd.device import Context
    assert callable(Context.debug_fill_idle) and not hasattr(microaligner_amd, "debug_fill_idle")
    assert "debug_fill_idle" not in getattr(microaligner_amd, "__all__", ())


def test_the_hook_refuses_a_null_context_and_a_byte_out_of_range_without_a_device():
    from microaligner_amd import _lib
    lib = _lib.load()
    filled = (C.c_ulonglong * 4)(7, 7, 7, 7)
    assert lib.ma_debug_fill_idle(None, 0, filled) == _lib.MA_EINVAL
    assert list(filled) == [7, 7, 7, 7]
    from microaligner_amd.device import Context
    for bad in (-1, 256, 0.5, True, None, "0"):
        with pytest.raises(ValueError):
            Context.debug_fill_idle(object(), bad)          # refused before the context is looked at


def test_the_hook_stays_out_of_the_measured_path_hash(tmp_path, monkeypatch):
    """build.source_hash() names the kernels a profile measured: editing debug_fill.hip or its header must leave it unchanged,
    editing a measured-path source must change it."""
    from microaligner_amd import build
    assert "debug_fill.hip" in build.SOURCES and HEADER not in [os.path.abspath(h) for h in build.HEADERS]
    assert [os.path.abspath(h) for h in build.SOURCE_HEADERS["debug_fill.hip"]] == [HEADER]
    src = open(os.path.join(build.CSRC, "debug_fill.hip")).read()
    assert '#include "ma_internal.h"' in src and "__global__" not in src
    out = subprocess.run([sys.executable, "-c", "from microaligner_amd import build; print(build.source_hash())"], cwd=ROOT,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == build.source_hash() and re.fullmatch(r"[0-9a-f]{16}", out)
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == out
    with open(csrc / "debug_fill.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() == out
    os.remove(csrc / "debug_fill.hip")                       # not even read
    assert build.source_hash() == out
    with open(csrc / "ma_api.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() != out


# ---- completeness of the registry ----------------------------------------------------------------------------------------------
# what EXEMPT may hold: context, option, event, engine and profile calls, allocation and copies of caller memory, host memory
# and host arithmetic, device queries, and the few named entries that launch no kernel over scratch memory
EXEMPT_PREFIXES = ("ma_ctx_", "ma_event_", "ma_engine_", "ma_profile_", "ma_memcpy_", "ma_host_", "ma_device_")
EXEMPT_NAMES = {"ma_sync", "ma_malloc", "ma_free", "ma_memset", "ma_version", "ma_last_error", "ma_clock_probe",
                "ma_params_default", "ma_warp_pages_plan", "ma_debug_fill_idle",
                # host only, no ctx argument: counters of the page-locking of caller memory; arithmetic on a table of moments
                "ma_transient_pin_stats", "ma_translation_scores"}


def all_entries():
    from microaligner_amd import _lib
    tables = {n: d for n, d in vars(_lib).items() if n.endswith("SIGNATURES") and isinstance(d, dict)}
    assert len(tables) >= 20 and "SIGNATURES" in tables and "DEBUG_SIGNATURES" in tables
    return {name: sig for d in tables.values() for name, sig in d.items()}


def test_every_entry_is_exercised_on_stale_memory_or_exempt():
    entries = all_entries()
    declared = S.declared_entries()
    assert not declared - set(entries), f"cases declare entries the bindings do not have: {sorted(declared - set(entries))}"
    assert not set(S.EXEMPT) - set(entries), f"EXEMPT names entries the bindings do not have: {sorted(set(S.EXEMPT) - set(entries))}"
    both = declared & set(S.EXEMPT)
    assert not both, f"exercised and exempt at once: {sorted(both)}"
    missing = set(entries) - declared - set(S.EXEMPT)
    assert not missing, f"neither exercised on stale scratch memory nor exempt: {sorted(missing)}"
    assert declared | set(S.EXEMPT) == set(entries)


def test_exempt_holds_no_compute_entry():
    entries = all_entries()
    for name, reason in S.EXEMPT.items():
        assert isinstance(reason, str) and reason.strip(), name
        assert name in EXEMPT_NAMES or name.startswith(EXEMPT_PREFIXES), f"{name} is a compute entry: it needs a case"
    # the two host-only entries beyond the prefixes take no context at all
    for name in ("ma_transient_pin_stats", "ma_translation_scores", "ma_warp_pages_plan"):
        assert entries[name][1][0] is not C.c_void_p or name == "ma_transient_pin_stats"
    src = open(os.path.join(ROOT, "microaligner_amd", "csrc", "translation.hip")).read()
    body = src[src.index("int ma_translation_scores("):]
    assert "ctx" not in body[:body.index("\n}\n")]


def test_cases_are_named_once_and_declare_entries():
    names = [c.name for c in S.CASES]
    assert len(names) == len(set(names)) and len(names) > 80
    for c in S.CASES:
        assert c.entries and all(isinstance(e, str) and e.startswith("ma_") for e in c.entries), c.name
        assert callable(c.make)
