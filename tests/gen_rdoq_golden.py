"""Writes tests/golden/rdoq.npz: the TUs of tests/rdoq_cases.py with what the compiled reference's own kvz_rdoq leaves in dest_coeff
(tests/ref_rdoq.py), the context sets and the processed quant_coeff / error_scale tables of flat and default lists.  Numeric arrays only.
Run from the repository root after build():  python tests/gen_rdoq_golden.py

Refuses to write unless the model (tests/rdoq_model.py) agrees with the reference on every TU, the reference wrote every value of every
dest, every census class is reached on at least MIN_PER_CLASS TUs, every deliberate error of the model changes at least one stored
result, and the file is no larger than the largest fixture already in tests/golden/."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rdoq_cases as K          # noqa: E402
import rdoq_model as M          # noqa: E402
import ref_rdoq as R            # noqa: E402

OUT = os.path.join(HERE, "golden", "rdoq.npz")
MIN_PER_CLASS = 4


def main():
    assert R.available(), "the compiled reference is missing: run build() where the reference's source is"
    assert R.entropy_bits() == list(M.ENTROPY_BITS)
    assert R.ctx_offsets() == (M.ROOT_CBF, M.QT_CBF_LUMA, M.QT_CBF_CHROMA, 32)
    base = K.base_contexts(R.init_contexts)
    dumps, qps, lambdas = K.context_sets(base)
    tables = [R.packed_tables(sl) for sl in (0, 1)]
    cs = K.cases()
    coeffs, desc = K.pack(cs)
    dest = np.zeros_like(coeffs)
    census = collections.Counter()
    differs_from_rounding = sign_hiding_changes = 0
    for i, (c, width, type_, scan, block_type, tr_depth, set_, cfg) in enumerate(cs):
        signhide, sl = K.CONFIGS[cfg]
        want = R.rdoq(c, width, type_, scan, block_type, tr_depth, int(qps[set_]), float(lambdas[set_]), dumps[set_], signhide, sl)
        assert not (want == np.int16(R.CANARY)).any(), "the reference left part of dest unwritten on TU %d" % i
        quant, err = tables[sl]
        got = M.rdoq(c.tolist(), width, type_, scan, block_type, tr_depth, int(qps[set_]), float(lambdas[set_]), dumps[set_].tolist(), quant, err,
                     signhide, census=census)
        assert got == want.tolist(), "model and reference differ on TU %d (width %d type %d scan %d set %d cfg %d)" % (i, width, type_, scan, set_, cfg)
        dest[desc[i, 0]:desc[i, 0] + c.size] = want
        if signhide:
            plain = R.rdoq(c, width, type_, scan, block_type, tr_depth, int(qps[set_]), float(lambdas[set_]), dumps[set_], 0, sl)
            sign_hiding_changes += int((plain != want).any())
    short = {k: census[k] for k in M.CLASSES if census[k] < MIN_PER_CLASS}
    assert not short, "census classes reached on fewer than %d TUs: %r" % (MIN_PER_CLASS, short)
    missed = []
    for name in M.MUTANTS:
        for i, (c, width, type_, scan, block_type, tr_depth, set_, cfg) in enumerate(cs):
            signhide, sl = K.CONFIGS[cfg]
            quant, err = tables[sl]
            got = M.rdoq(c.tolist(), width, type_, scan, block_type, tr_depth, int(qps[set_]), float(lambdas[set_]), dumps[set_].tolist(), quant, err,
                         signhide, mutant=name)
            if got != dest[desc[i, 0]:desc[i, 0] + c.size].tolist():
                break
        else:
            missed.append(name)
    assert not missed, "deliberate errors that change no stored result: %r" % missed
    np.savez_compressed(OUT, coeffs=coeffs, desc=desc.astype(np.uint32), dest=dest, base_ctx=base, dumps=dumps, qps=qps, lambdas=lambdas,
                        quant=np.stack([t[0] for t in tables]), err_scale=np.stack([t[1] for t in tables]),
                        configs=np.array(K.CONFIGS, dtype=np.int32), census=np.array([census[k] for k in M.CLASSES], dtype=np.int32))
    size = os.path.getsize(OUT)
    largest = max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden")) if f != "rdoq.npz")
    assert size <= largest and size < (1 << 20), "%d bytes" % size
    print("%s: %d TUs, %d bytes; sign hiding changes %d TUs" % (OUT, len(cs), size, sign_hiding_changes))
    for k in M.CLASSES:
        print("  %-40s %d" % (k, census[k]))


if __name__ == "__main__":
    main()
