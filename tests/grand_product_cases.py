"""Shared by tests/test_grand_product_cpu.py and tests/test_gpu_grand_product.py: the reference's messages as a package Proof,
and the list of single tampers with the error each must meet."""
import grand_product_ref as ref

GOLD = 2**64 - 2**32 + 1
P64 = 2**64 - 59
P61 = 2**61 - 1


mont_list = ref.mont_list


def ref_proof(pkg, t_canon, p, challenges_canon=None, draw=None):
    """the reference prover over canonical t under fixed canonical challenges (protocol order) or a canonical draw, as a package
    Proof in Montgomery words"""
    it = iter(challenges_canon) if challenges_canon is not None else None
    out = ref.prove(t_canon, p, draw if draw is not None else (lambda k, j, msg: next(it)))
    gp = pkg.grand_product
    return gp.Proof(ref.mont(out["product"], p), [[mont_list(m, p) for m in layer] for layer in out["rounds"]],
                    [tuple(mont_list(f, p)) for f in out["finals"]], mont_list(out["point"], p), ref.mont(out["claim"], p),
                    mont_list(out["challenges"], p))


def n_challenges(n):
    return n * (n - 1) // 2 + n


def tampers(n):
    """(name, where, expected) for a proof of n >= 3 layers: where = ("product",) | ("round", k, j, t) | ("final", k, side);
    expected = ("product",) | ("round", k, j) | ("final", k).  A round is tampered in the first layer that has one (its only
    round), in a middle layer (a middle round) and in the last layer (its last round); values 0 and 1 break the round's own sum,
    values 2 and 3 the claim it hands on - to the next round, or to the finals after a layer's last round"""
    out = [("product", ("product",), ("product",))]
    for k, j in ((1, 0), (n // 2, (n // 2) // 2), (n - 1, n - 2)):
        for t in range(4):
            if t < 2:
                expected = ("round", k, j)
            elif j + 1 < k:
                expected = ("round", k, j + 1)
            else:
                expected = ("final", k)
            out.append(("L%d_R%d_H%d" % (k, j, t), ("round", k, j, t), expected))
    for k in range(n):
        for side in range(2):
            out.append(("L%d_final%d" % (k, side), ("final", k, side), ("product",) if k == 0 else ("final", k)))
    return out


def apply_tamper(pkg, proof, where, F):
    """the proof with one word changed (+ 1)"""
    bump = lambda w: F.add(int(w), F.one)   # noqa: E731
    product, rounds, finals = proof.product, [[list(m) for m in layer] for layer in proof.rounds], [list(f) for f in proof.finals]
    if where[0] == "product":
        product = bump(product)
    elif where[0] == "round":
        _, k, j, t = where
        rounds[k][j][t] = bump(rounds[k][j][t])
    else:
        _, k, side = where
        finals[k][side] = bump(finals[k][side])
    return proof._replace(product=product, rounds=rounds, finals=[tuple(f) for f in finals])


def expect_refusal(pkg, verifier, proof, challenges, expected):
    """verifier.verify(proof, challenges) must raise exactly the error `expected` names"""
    import pytest
    gp = pkg.grand_product
    kind = {"product": gp.ProductMismatch, "round": gp.RoundMismatch, "final": gp.FinalMismatch}[expected[0]]
    with pytest.raises(kind) as ei:
        verifier.verify(proof, challenges)
    assert type(ei.value) is kind
    if expected[0] == "round":
        assert (ei.value.layer, ei.value.round) == expected[1:]
    elif expected[0] == "final":
        assert ei.value.layer == expected[1]
