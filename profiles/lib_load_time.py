"""Start-up cost of the binding: N fresh processes, each with torch already imported, time `from sfh_amd import _lib`
(which reads include/sfh_amd.h) and `_lib.load()` (dlopen + binding every symbol).  No device needed.
    python profiles/lib_load_time.py [N]          # one line of milliseconds per process, then the medians"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = ("import sys, time; sys.path.insert(0, %r); import torch, ctypes, re\n"
         "t0 = time.perf_counter(); from sfh_amd import _lib; t1 = time.perf_counter(); _lib.load(); t2 = time.perf_counter()\n"
         "print((t1 - t0) * 1e3, (t2 - t1) * 1e3)\n" % ROOT)

rows = []
for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 7):
    out = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, check=True).stdout
    rows.append([float(v) for v in out.split()])
    print("import %.1f ms   load %.1f ms" % tuple(rows[-1]))
print("median: import %.1f ms   load %.1f ms" % tuple(statistics.median(c) for c in zip(*rows)))
