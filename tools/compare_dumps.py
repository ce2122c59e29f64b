"""Compare two `bench.py --dump-outputs` directories array for array with numpy.array_equal (bit for bit; NaNs in the same
places count as equal).  Exits non-zero on any difference, on a file missing from either side, or when there is nothing to compare.
python tools/compare_dumps.py DIR_A DIR_B [label]"""
import os, sys
import numpy as np
da, db = sys.argv[1], sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else "%s vs %s" % (da, db)
fa = sorted(f for f in os.listdir(da) if f.endswith(".npy"))
fb = sorted(f for f in os.listdir(db) if f.endswith(".npy"))
bad = sorted(set(fa) ^ set(fb))
for f in bad:
    print("%s: %s only on one side" % (label, f))
for f in sorted(set(fa) & set(fb)):
    a, b = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
    same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    print("%s: %-20s %-8s %-14s %s" % (label, f, a.dtype, a.shape, "equal" if same else "DIFFERENT (%d entries)" % (
        int((a != b).sum()) if a.shape == b.shape else -1)))
    if not same:
        bad.append(f)
if not fa or not fb:
    print("%s: nothing to compare" % label)
    sys.exit(2)
print("%s: %s" % (label, "ALL EQUAL (%d arrays)" % len(fa) if not bad else "%d DIFFERENCE(S)" % len(bad)))
sys.exit(1 if bad else 0)
