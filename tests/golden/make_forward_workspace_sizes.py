"""Record the forward path's three workspace size queries: python make_forward_workspace_sizes.py PATH/TO/libwakeword_amd.so

Run it on a build of the commit BEFORE a change to the workspace layout, never on the code under test: tests/test_host_workspaces.py
compares the library it tests with this record.  The queries are host arithmetic; no GPU is needed.  The grid is the one of
tests/test_host_workspaces.py (NS x SAMPLES x n_conv); keys are "n,n_conv" and "n,n_samples,n_conv"."""
import ctypes as C
import itertools
import json
import os
import sys

NS = (0, 1, 2, 5, 16, 17, 255, 256, 257, 4096)
SAMPLES = (4000, 4096, 8000, 12345, 16000, 16383, 16384, 24000, 32000)

lib = C.CDLL(sys.argv[1])
for name, argtypes in (("ww_workspace_bytes", [C.c_int64, C.c_int32]), ("ww_workspace_frames_bytes", [C.c_int64, C.c_int64, C.c_int32]),
                       ("ww_forward_windows_workspace_bytes", [C.c_int64, C.c_int64, C.c_int32])):
    getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int64, argtypes
sizes = {"ww_workspace_bytes": {f"{n},{c}": lib.ww_workspace_bytes(n, c) for n, c in itertools.product(NS, (2, 3))}}
for name in ("ww_workspace_frames_bytes", "ww_forward_windows_workspace_bytes"):
    sizes[name] = {f"{n},{s},{c}": getattr(lib, name)(n, s, c) for n, s, c in itertools.product(NS, SAMPLES, (2, 3))}
assert all(v >= 0 for table in sizes.values() for v in table.values())
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "forward_workspace_sizes.json"), "w") as f:
    json.dump(sizes, f, indent=0, sort_keys=True)
    f.write("\n")
