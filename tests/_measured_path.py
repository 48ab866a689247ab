"""The measured path's source hash, stated once for the tests that pin it.

microaligner_amd.build.source_hash() is taken over the sources and headers of the kernels that bench.py measures; a profile or
a benchmark figure is valid for the tree whose hash it names.  The tests of every feature that must stay off that path assert
that the hash is still this value, and some that the loaded library was built from it.

A pull request changes the value only when it changes a measured-path source on purpose -- then here, in the same commit, and
with a fresh benchmark figure beside the parent's.  A feature that is meant to leave the measured path alone and finds this
value changed has touched that path by accident."""
HASH = "c8c3e3bfcfe3f943"
