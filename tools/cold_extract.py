"""cold_extract.py: first orbx_extract of a fresh context at 1241 x 376 (plan + uploads + workspace + the frame), after the runtime and the code
objects have been warmed by another context at another shape.  Prints the five times in ms."""
import os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ceres_mono_orb_slam2_amd import ORBextractor, synth
warm = ORBextractor(1000, 1.2, 8, 20, 7)
for _ in range(3): warm(synth.make_frame(0, 640, 480, "blocks"))
img = synth.make_frame(1, 1241, 376, "blocks")
ts = []
for i in range(5):
    ex = ORBextractor(2000, 1.2, 8, 20, 7)
    t0 = time.perf_counter(); k, d = ex(img); ts.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter(); ex(img); warm_ms = (time.perf_counter() - t0) * 1e3
    del ex
print(json.dumps({"cold_extract_ms": [round(t, 3) for t in ts], "second_call_ms": round(warm_ms, 3), "keypoints": len(k)}))
