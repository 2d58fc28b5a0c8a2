"""Generate the fp8 golden fixtures by running the UNMODIFIED reference kvcompress on the exact
bf16 upcast of fp8 keys (build container only).

    cd <repo> && PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_fp8_goldens.py

The reference cannot run on fp8 tensors (torch.norm / torch.gather are not implemented for them),
and the engine's contract for an fp8 cache is defined through the upcast: the kept positions are
those the reference method keeps on K8.to(torch.bfloat16), and the output is the fp8 BYTES of K
and V at those positions.  So per case this script

  * builds K8 / V8 from tests/fp8_util.py's recipe (prng's splitmix64 normals, quantised to fp8 by
    an explicit round-to-nearest-even in numpy; input hashes stored to detect drift),
  * runs the reference method on (K8.to(bfloat16), V encoding its own positions) and reads the kept
    source position of every output row back,
  * stores those positions per layer and the SHA-256 of the expected fp8 K / V output bytes.

Nothing of the reference is copied; outputs (data only): fp8_cases.json, fp8_positions.npz.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))           # tests/: fp8_util
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repo root: oracle (fp8_util's import)
import prng  # noqa: E402
import fp8_util as F  # noqa: E402

import kvcompress  # noqa: E402,F401  (the reference: first on PYTHONPATH)
from kvcompress.methods import get_compress_fn  # noqa: E402

assert not hasattr(kvcompress, "_native"), "run with PYTHONPATH=<the reference>, not the engine"
torch.set_num_threads(8)

SHAPE = (1, 2, 1500, 128)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cases():
    out = []
    seed = 8800
    for method in F.METHODS:
        kwargs = F.ORACLE_METHODS[method][1]
        for fmt in F.FORMATS:
            seed += 3
            out.append(dict(id=f"{method}_{fmt}", method=method, fmt=fmt, kwargs=kwargs,
                            layers=[dict(shape=list(SHAPE), kseed=seed + i, variant="normal")
                                    for i in range(3)]))
    # tie-heavy rows (three distinct norms), and NaN / zero / (e5m2) inf rows
    for fmt in F.FORMATS:
        seed += 3
        out.append(dict(id=f"fix_size_l2_{fmt}_few", method="fix_size_l2", fmt=fmt,
                        kwargs=F.ORACLE_METHODS["fix_size_l2"][1],
                        layers=[dict(shape=list(SHAPE), kseed=seed + i, variant="few")
                                for i in range(3)]))
    for fmt in F.FORMATS:
        seed += 3
        out.append(dict(id=f"h2o_l2_{fmt}_special", method="h2o_l2", fmt=fmt,
                        kwargs=F.ORACLE_METHODS["h2o_l2"][1],
                        layers=[dict(shape=list(SHAPE), kseed=seed + i, variant="special")
                                for i in range(3)]))
    return out


def bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def main():
    meta, positions = [], {}
    for c in cases():
        fmt = c["fmt"]
        ks = [F.gen_keys(L["kseed"], tuple(L["shape"]), fmt, L["variant"]) for L in c["layers"]]
        vs = [F.gen_values(L["kseed"], tuple(L["shape"]), fmt) for L in c["layers"]]
        t8 = F.torch_dtype(fmt)
        layers = []
        for k in ks:
            k16 = torch.from_numpy(k).view(t8).to(torch.bfloat16)  # the contract's upcast
            got = k16.view(torch.int16).numpy().view(np.uint16)
            nan = np.isin(k, F.NAN_CODES[fmt])  # (a NaN's sign / payload decide nothing)
            assert np.array_equal(got[~nan], F.to_bf16_bits(k, fmt)[~nan])
            layers.append((k16, bf16_tensor(prng.encode_positions(k.shape, "bf16"))))
        with torch.no_grad():
            out = get_compress_fn(c["method"])(layers, **c["kwargs"])
        rec = dict(c, layers_out=[])
        for i, (_, v_out) in enumerate(out):
            v_np = v_out.contiguous().view(torch.int16).numpy().view(np.uint16)
            pos, ok = prng.decode_positions(v_np, "bf16")
            assert ok, c["id"]
            positions[f"{c['id']}/{i}"] = pos.astype(np.uint16)
            rec["layers_out"].append(dict(
                n_out=int(pos.shape[2]), k_input_sha=sha(ks[i]), v_input_sha=sha(vs[i]),
                k_sha=sha(F.take_rows(ks[i], pos)), v_sha=sha(F.take_rows(vs[i], pos))))
        meta.append(rec)
        print(c["id"], [r["n_out"] for r in rec["layers_out"]])
    with open(os.path.join(HERE, "fp8_cases.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "fp8_positions.npz"), **positions)


if __name__ == "__main__":
    main()
