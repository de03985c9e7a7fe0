"""Writes tests/golden/coeff_cabac.npz: the TUs of tests/coeff_cabac_cases.py with the counts of the compiled reference's own counting coder
(tests/ref_coeff_cost.py).  Run from the repository root after build():  python tests/gen_coeff_cabac_golden.py

Refuses to write unless the model (tests/coeff_cabac_model.py) agrees with the reference on every TU, every census class is reached on at
least MIN_PER_CLASS TUs, and every deliberate error of the model changes at least one stored count."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import coeff_cabac_cases as K          # noqa: E402
import coeff_cabac_model as M          # noqa: E402
import ref_coeff_cost as R             # noqa: E402

OUT = os.path.join(HERE, "golden", "coeff_cabac.npz")
MIN_PER_CLASS = 4
MAX_BYTES = 400 * 1000


def main():
    assert R.available(), "the compiled reference is missing: run build() where the reference's source is"
    for width in (4, 8, 16, 32):
        for mode in ((0, 1, 2) if width <= 8 else (0,)):
            assert R.scan_table(width, mode) == M.scan_tables(width, mode)[0], (width, mode)
    ranges, dumps = K.context_sets()
    cs = K.cases()
    bits = np.zeros(len(cs), dtype=np.uint32)
    census = collections.Counter()
    for i, (c, width, type_, scan, tr_skip, set_, cfg) in enumerate(cs):
        sh, ts, ll = K.CONFIGS[cfg]
        want, after = R.coeff_cabac_cost(c, width, type_, scan, int(ranges[set_]), dumps[set_], sh, ts, ll, tr_skip)
        got = M.count_bits(c.tolist(), width, type_, scan, tr_skip, int(ranges[set_]), dumps[set_].tolist(), sh, ts, ll, census=census)
        assert got == want, "model %d, reference %d on TU %d (width %d type %d scan %d)" % (got, want, i, width, type_, scan)
        bits[i] = want
    short = {k: census[k] for k in M.CLASSES if census[k] < MIN_PER_CLASS}
    assert not short, "census classes reached on fewer than %d TUs: %r" % (MIN_PER_CLASS, short)
    for name in M.MUTANTS:
        hit = 0
        for i, (c, width, type_, scan, tr_skip, set_, cfg) in enumerate(cs):
            sh, ts, ll = K.CONFIGS[cfg]
            if M.count_bits(c.tolist(), width, type_, scan, tr_skip, int(ranges[set_]), dumps[set_].tolist(), sh, ts, ll, mutant=name) != bits[i]:
                hit += 1
                break
        assert hit, "deliberate error %r changes no stored count" % name
    coeffs, desc = K.pack(cs)
    np.savez_compressed(OUT, coeffs=coeffs, desc=desc.astype(np.uint32), ranges=ranges, dumps=dumps, bits=bits,
                        configs=np.array(K.CONFIGS, dtype=np.int32), census=np.array([census[k] for k in M.CLASSES], dtype=np.int32))
    size = os.path.getsize(OUT)
    assert size < MAX_BYTES, "%d bytes" % size
    print("%s: %d TUs, %d bytes, bits %d..%d" % (OUT, len(cs), size, bits[bits > 0].min(), bits.max()))


if __name__ == "__main__":
    main()
