"""The core of the registry of GPU cases: what a case is, the list the area modules of this package append to, the C
entries no case needs to exercise, what make() is handed, the bit-for-bit comparison, and the input helpers the cases
share.  Nothing here needs a GPU, the oracle build or a test module; what a case needs it imports inside make()."""
import numpy as np

F32, F64 = np.float32, np.float64
POISONS = (0xFF, 0x7F, 0x00)


# C entries that launch no kernel over scratch memory: the cap on what the registry may leave out
EXEMPT = {
    "ma_version": "a string",
    "ma_last_error": "a string",
    "ma_device_count": "device query",
    "ma_device_info": "device query",
    "ma_ctx_create": "context call",
    "ma_ctx_destroy": "context call",
    "ma_ctx_stream": "context call",
    "ma_ctx_trim": "context call: frees the caches",
    "ma_ctx_transfer_stats": "context call: reads two host counters",
    "ma_ctx_set_workspace_limit": "option call",
    "ma_ctx_set_option": "option call",
    "ma_ctx_get_option": "option call",
    "ma_sync": "context call: waits for the stream",
    "ma_malloc": "allocation",
    "ma_free": "allocation",
    "ma_memset": "fills caller memory",
    "ma_memcpy_h2d": "copy between caller buffers",
    "ma_memcpy_d2h": "copy between caller buffers",
    "ma_memcpy_d2d": "copy between caller buffers",
    "ma_memcpy_d2h_async": "copy between caller buffers",
    "ma_host_alloc": "host memory",
    "ma_host_free": "host memory",
    "ma_host_register": "host memory",
    "ma_host_unregister": "host memory",
    "ma_host_transfer_is_direct": "host memory query",
    "ma_host_parallel_copy": "host copy",
    "ma_host_stream_copy": "host copy",
    "ma_host_pcg64_choice2": "host arithmetic, no ctx",
    "ma_host_ransac_iterations": "host arithmetic, no ctx",
    "ma_host_np_mean": "host arithmetic, no ctx",
    "ma_transient_pin_stats": "host counters of the page-locking of caller memory, no ctx",
    "ma_translation_scores": "host arithmetic on a table of moments, no ctx (include/microaligner_translation.h)",
    "ma_event_create": "event call",
    "ma_event_destroy": "event call",
    "ma_event_record": "event call",
    "ma_event_elapsed_ms": "event call",
    "ma_event_sync": "event call",
    "ma_engine_memcpy_h2d": "engine call: copy between caller buffers through the staging rings",
    "ma_engine_memcpy_d2h": "engine call: copy between caller buffers through the staging rings",
    "ma_engine_record": "engine call",
    "ma_engine_wait": "engine call",
    "ma_engine_sync": "engine call",
    "ma_profile_enable": "profile call",
    "ma_profile_reset": "profile call",
    "ma_profile_get": "profile call",
    "ma_clock_probe": "a spin kernel that touches no memory",
    "ma_params_default": "fills a host struct",
    "ma_warp_pages_plan": "host arithmetic, no ctx",
    "ma_debug_fill_idle": "the hook itself",
}


class Case:
    """name; the C entries the case exercises; make(env) -> (run, expected): run() makes the call(s) and returns the
    results as numpy arrays / scalars in tuples, lists or dicts; expected is the same structure (compared bit for bit, NaN
    standing for NaN) or a function check(result) where the primitive's own test uses a tolerance.  bits: whether the four
    results must be bit-identical to each other."""

    def __init__(self, name, entries, make, bits=True):
        self.name, self.entries, self.make, self.bits = name, tuple(entries), make, bits


CASES = []


def case(name, entries, bits=True):
    if isinstance(entries, str):
        entries = (entries,)

    def deco(make):
        assert name not in [c.name for c in CASES], name
        CASES.append(Case(name, entries, make, bits))
        return make
    return deco


def declared_entries():
    return {e for c in CASES for e in c.entries}


class Env:
    """what make() gets: the context, and the restatements that are compiled once per module"""

    def __init__(self, ctx, tmp_path_factory):
        self.ctx, self._tmp, self._made = ctx, tmp_path_factory, {}
        self.poison = POISONS[0]         # the byte Context.empty and the cases' host outputs are filled with

    def _once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    @property
    def interp(self):
        from _remap_interp_ref import InterpRef
        return self._once("interp", lambda: InterpRef(self._tmp.mktemp("stale_interp_ref")))

    @property
    def levels(self):
        from _fb_levels_ref import LevelsRef
        return self._once("levels", lambda: LevelsRef(self._tmp.mktemp("stale_levels_ref")))


def assert_same(got, exp, where=""):
    """the same structure and the same bits, any NaN payload standing for NaN"""
    if isinstance(exp, dict):
        assert isinstance(got, dict) and set(got) == set(exp), where
        for k in exp:
            assert_same(got[k], exp[k], f"{where}[{k!r}]")
    elif isinstance(exp, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(exp), where
        for k, (g, e) in enumerate(zip(got, exp)):
            assert_same(g, e, f"{where}[{k}]")
    elif exp is None:
        assert got is None, where
    elif isinstance(exp, np.ndarray):
        # float arrays by their bits, hence of one dtype; integer and bool arrays by their values (flags come back as bool)
        assert isinstance(got, np.ndarray) and got.shape == exp.shape and \
            (got.dtype == exp.dtype or "f" not in (got.dtype.kind, exp.dtype.kind)), \
            f"{where}: {getattr(got, 'dtype', type(got))} {getattr(got, 'shape', None)} against {exp.dtype} {exp.shape}"
        if exp.dtype.kind == "f":
            gn, en = np.isnan(got), np.isnan(exp)
            assert np.array_equal(gn, en), f"{where}: NaN masks differ at {np.argwhere(gn != en)[:5].tolist()}"
            u = {4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
            bad = np.ascontiguousarray(got).view(u) != np.ascontiguousarray(exp).view(u)
            bad &= ~en
        else:
            bad = got != exp
        assert not bad.any(), f"{where}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[:5].tolist()}"
    elif isinstance(exp, (float, np.floating)):
        assert (got == exp) or (got != got and exp != exp), f"{where}: {got!r} against {exp!r}"
    else:
        assert got == exp, f"{where}: {got!r} against {exp!r}"


# ---- inputs --------------------------------------------------------------------------------------------------------------
SHAPE = (67, 301)       # ragged against every tile of the library, more than one block along x


def pair(h, w, seed, dtype=np.float32, **kw):
    from microaligner_amd import synthetic
    return synthetic.make_pair(h, w, seed, dtype, **kw)


def labels_u8(h, w, seed):
    """random labels over all 256 values"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def dev(ctx, *arrays):
    out = tuple(None if a is None else ctx.asdevice(a) for a in arrays)
    return out[0] if len(out) == 1 else out


def _O():
    from oracle import oracle as O
    return O


def _RO():
    from oracle import register_oracle as RO
    return RO
