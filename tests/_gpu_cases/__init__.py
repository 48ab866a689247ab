"""The registry of GPU cases: one small call per C entry of the bindings that launches a kernel, with its inputs and the
result its statement gives.

tests/test_gpu_stale_memory.py runs every case on stale scratch memory and tests/test_gpu_unaligned.py at unaligned device
addresses; tests/test_debug_fill.py (no GPU) checks that the entries the cases declare and EXEMPT together are every entry of
the bindings.  registry.py holds what a case is and what the cases share; every other module holds the cases of one area and
registers them with @case when it is imported.  CASES keeps the order of the imports below, which is the order the two
parametrised tests run in.

Cases for a new entry: one new module here and one import line below.  Importing the package needs no GPU, no oracle build
and no test module -- a case imports those inside make().  A test module that imports the package calls
pytest.register_assert_rewrite("_gpu_cases") first, so that the asserts of the cases report their operands."""
from .registry import (CASES, EXEMPT, POISONS, SHAPE, Case, Env, _O, _RO, assert_same, case, declared_entries, dev,  # noqa: F401
                       labels_u8, pair)
# the area modules, in the order of CASES: not to be sorted
from . import farneback, pyramid, dog, gate, warps, flows, features, whole_path, local_norm  # noqa: F401
