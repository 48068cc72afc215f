"""Shared by tests/test_logup_cpu.py and tests/test_gpu_logup.py: the reference's messages as a package Proof, and the list of
single tampers with the error each must meet."""
import logup_ref as ref

GOLD = 2**64 - 2**32 + 1
P64 = 2**64 - 59
P61 = 2**61 - 1


mont_list = ref.mont_list
n_challenges = ref.n_challenges


def as_proof(pkg, out, p):
    """a reference prove() dict (canonical) as a package Proof in Montgomery words"""
    return pkg.logup.Proof(tuple(mont_list(out["root"], p)), [[mont_list(m, p) for m in layer] for layer in out["rounds"]],
                           [tuple(mont_list(f, p)) for f in out["finals"]], mont_list(out["point"], p), tuple(mont_list(out["claims"], p)),
                           mont_list(out["challenges"], p))


def ref_proof(pkg, pt, qt, p, challenges_canon=None, draw=None):
    """the reference prover over canonical tables (pt None: all ones) under fixed canonical challenges (in the order they are
    drawn) or a canonical draw, as a package Proof"""
    it = iter(challenges_canon) if challenges_canon is not None else None
    return as_proof(pkg, ref.prove(pt, qt, p, draw if draw is not None else (lambda k, j, msg: next(it))), p)


def lambda_index(k):
    """where lambda_k, k >= 1, stands among the challenges as drawn: rho_0, then per layer j >= 1 lambda_j, j rounds, rho_j"""
    return 1 + sum(j + 2 for j in range(1, k))


def tampers(n):
    """(name, where, expected) for a proof of n >= 3 layers: where = ("root", side) | ("round", k, j, t) | ("final", k, which) |
    ("lambda", k); expected = ("root",) | ("round", k, j) | ("final", k).  A round is tampered in the first layer that has one (its
    only round), in a middle layer (a middle round) and in the last layer (its last round); values 0 and 1 break the round's own
    sum, values 2 and 3 the claim it hands on - to the next round, or to the finals after a layer's last round.  A changed lambda
    changes the claim a + lambda b that the layer's first round must meet"""
    out = [("root_P", ("root", 0), ("root",)), ("root_Q", ("root", 1), ("root",))]
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
        for which in range(4):
            out.append(("L%d_final%d" % (k, which), ("final", k, which), ("root",) if k == 0 else ("final", k)))
    for k in sorted({1, n // 2, n - 1}):
        out.append(("lambda%d" % k, ("lambda", k), ("round", k, 0)))
    return out


def apply_tamper(pkg, proof, where, F):
    """(proof, challenges) with one word changed (+ 1)"""
    bump = lambda w: F.add(int(w), F.one)   # noqa: E731
    root, rounds, finals = list(proof.root), [[list(m) for m in layer] for layer in proof.rounds], [list(f) for f in proof.finals]
    challenges = list(proof.challenges)
    if where[0] == "root":
        root[where[1]] = bump(root[where[1]])
    elif where[0] == "round":
        _, k, j, t = where
        rounds[k][j][t] = bump(rounds[k][j][t])
    elif where[0] == "final":
        _, k, which = where
        finals[k][which] = bump(finals[k][which])
    else:
        at = lambda_index(where[1])
        challenges[at] = bump(challenges[at])
    return proof._replace(root=tuple(root), rounds=rounds, finals=[tuple(f) for f in finals]), challenges


def expect_refusal(pkg, verifier, proof, challenges, expected):
    """verifier.verify(proof, challenges) must raise exactly the error `expected` names"""
    import pytest
    lu = pkg.logup
    kind = {"root": lu.RootMismatch, "round": lu.RoundMismatch, "final": lu.FinalMismatch}[expected[0]]
    with pytest.raises(kind) as ei:
        verifier.verify(proof, challenges)
    assert type(ei.value) is kind
    if expected[0] == "round":
        assert (ei.value.layer, ei.value.round) == expected[1:]
    elif expected[0] == "final":
        assert ei.value.layer == expected[1]
