import sys, os, numpy as np
a, b, label = sys.argv[1], sys.argv[2], sys.argv[3]
for f in sorted(os.listdir(a)):
    if not f.endswith('.npy') or not os.path.exists(os.path.join(b, f)):
        continue
    x, y = np.load(os.path.join(a, f)).astype(np.float64), np.load(os.path.join(b, f)).astype(np.float64)
    if x.shape != y.shape:
        print(label, f, 'shape', x.shape, y.shape); continue
    d = np.abs(x - y).max() if x.size else 0.0
    print('%s %s n=%d max|a-b|=%.3e rel_to_max=%.3e bitwise_equal=%s' % (label, f, x.size, d, d / max(np.abs(x).max(), 1e-30) if x.size else 0.0, np.array_equal(x, y)))
