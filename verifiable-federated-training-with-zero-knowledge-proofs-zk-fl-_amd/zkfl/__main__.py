"""Command line: the circom + snarkjs commands the reference harness runs, on this framework.

    python -m zkfl compile <circuit> [params..] [-o DIR]    circom <c>.circom --r1cs --wasm
        -> DIR/<name>.r1cs, DIR/<name>.zkwp (witness program: the .wasm's role)
        --circom-layout: also DIR/<name>_js/<name>.wasm (the witness-program image under circom's
        name) + DIR/<name>_js/generate_witness.cjs, so the harness's
        `node <name>_js/generate_witness.cjs <name>_js/<name>.wasm in.json out.wtns` runs unchanged
    python -m zkfl info <circuit> [params..]                 snarkjs r1cs info (tests/test_verified_gradient.mjs:351-356)
    python -m zkfl r1cs-info <file.r1cs>                     snarkjs r1cs info on a circom-compiled .r1cs
    python -m zkfl setup-r1cs <file.r1cs> [-o DIR]           snarkjs groth16 setup (+ contribute, export vk) on a
                                                             circom .r1cs (zkfl/r1cs_file.py); prove its circom
                                                             .wtns with `prove`
    python -m zkfl setup <circuit> [params..] [-o DIR]       snarkjs groth16 setup + zkey contribute + zkey export
        -> DIR/<name>_final.zkey, DIR/verification_key.json  verificationkey (tests/full_system_simulation.mjs:713-735)
                                                             DEVELOPMENT ceremony: fresh random toxic waste, discarded
    python -m zkfl export-vk <zkey> <vkey.json>              snarkjs zkey export verificationkey
    python -m zkfl wtns <circuit.zkwp> <input.json> <out.wtns>              generate_witness.cjs (:758-767)
    python -m zkfl wtns check <circuit.r1cs> <witness.wtns>                 snarkjs wtns check (alias: wchk); exit 1
                                                                            and the first failing constraint otherwise
    python -m zkfl prove <zkey> <wtns> <proof.json> <public.json> [--r1cs <circuit.r1cs>]   snarkjs groth16 prove
        (:773-776); --r1cs: check the witness first, exit 1 without writing a proof when it fails;
        --check-key <circuit.r1cs> <pot_final.ptau>: check the key first (as `zkey check`), the same way
    python -m zkfl zkey check <circuit.r1cs> <pot_final.ptau> <circuit.zkey>   is the key the circuit's Groth16 key over
        that prepared ptau, for some delta?  One line per check; exit 0, 1 when a check fails, 2 on
        unusable arguments (the reference trusts any `<c>_final.zkey` it finds, :713-738); --check-ptau:
        the ptau check below first
    python -m zkfl powersoftau check <pot.ptau>      is the file a well-formed Powers of Tau for some tau, alpha and
        beta, with sections 12-15 the Lagrange form of sections 2-5 (the reference takes any pot*_final.ptau
        it finds, :677-695)?  The same exit codes; an unprepared file passes on its powers alone
    python -m zkfl verify <vkey.json> <public.json> <proof.json>            snarkjs groth16 verify (:865-868)
    python -m zkfl verify-round <round.json>                 a round's `groth16 verify` calls (:1298-1343) as one
        verify_multi call.  round.json: a list of {"vkey": path, "public": path, "proof": path} (relative
        paths are taken from the manifest's directory); each distinct vkey is loaded once.  Prints one
        line per job, in job order; exit 0 if all are valid, 1 if any is invalid, 2 on a manifest that
        is not such a list or names a missing file (decided before the GPU is touched)
        --combined: answer the round by one random combination with one final exponentiation
        (verify_round; the per-proof path gives the verdicts when it fails).  Same lines and exit
        codes; the report goes to stderr
        --narrow: --combined, and when the combination fails the round is narrowed to the groups of jobs
        whose own combination fails; only those go to the per-proof path (verify_round_narrow).  Same
        lines and exit codes; the narrow report goes to stderr
    python -m zkfl aggregate-round <round.json>              aggregateUpdates (:1137-1199) with the masks of the
        excluded clients taken out.  round.json: {"round", "dim", "groups": [{"clients": [{"id",
        "accepted", "public"}], "revealed": [{"in", "out", "key"}]}]}; "public" is an accepted client's
        secure_masked_update public.json (client_id, round, ..., masked_update at signals 7..7+dim,
        :999-1000; relative paths are taken from the manifest's directory), "revealed" the pairwise key
        of every (accepted, excluded) pair of the group.  Prints one JSON line per group, {"group",
        "clients", "sum": [signed integers], "mean"}; exit 0, 1 if a group's sum is out of range (a mask
        is still in it), 2 on a manifest of another shape, a missing file, a public.json whose client_id
        or round disagrees with the manifest, a missing key or a key that is not needed (all decided
        before the GPU is touched)
    python -m zkfl admit-round <round.json>                  the server's decision between the two: the checks of
        verifyBalanceProof, verifyTrainingProof and verifySecureAggregationProof (:848-1131) before each
        `groth16 verify`, the proofs that pass them verified, in one call (zkfl/admit.py).  round.json:
        {"round", "tau_squared", "dim", "vkeys": {"balance", "training", "secagg": vkey.json paths},
        "weights": [dim values] (optional), "groups": [{"clients": [{"id", "balance": {"proof", "public",
        "root_D"}, "training": {"proof", "public", "root_D", "root_G", "root_W", "round", "gradient": [dim
        signed integers]}, "secagg": {"proof", "public", "root_D", "root_G", "root_W", "root_K", "round",
        "masked_update": [dim values]}, "peers": [ids] (optional)}], "revealed": [{"in", "out", "key"}]
        (optional)}]}; "proof" and "public" are proof.json / public.json paths (relative ones are taken
        from the manifest's directory), a client may lack any of its three packages, and a client's
        peers default to the other clients of its group in the group's order.  Prints one line per client
        and phase, `client <id> <phase>: OK` or the name of the first failing check (ZKFL_ADMIT_*,
        include/zkfl.h); exit 0 if every present package is accepted, 1 otherwise, 2 on a manifest of
        another shape, a missing file or a value that is not a canonical field element (decided before
        the GPU is touched)
        --reference: only the reference's checks (not: a package's round is the server's, root_W commits
        to "weights", the secagg proof's peer ids are the group's)
        --combined: as for verify-round
        --aggregate: then close each group over the clients whose secagg code is 0 (their masked updates
        are signals 7..7+dim of their public.json) with the group's "revealed" keys, and print
        aggregate-round's lines; a group without an accepted client prints "sum": null
    python -m zkfl prepare-round <manifest.json> -o DIR      the clients' half of a round (:1278-1343) in one call
        (zkfl/prepare.py): dataset trees and Merkle openings, fixed-point gradients, commitments and
        masked updates.  manifest.json: {"round", "tau_squared", "depth", "batch", "precision", "weights":
        [dim signed integers], "clients": [{"id", "features": [[dim integers] per sample], "labels": [0 or
        1 per sample], "batch_idx": [batch sample indices] (optional), "peers": [ids], "keys": [one per
        peer], "master_key"}]}; every client has the same shape, and "peers", "keys" and "master_key" may
        be absent from all of them (no secagg part).  "harness_keys": true instead of keys takes the
        harness's simulated keys (:1321-1336), every client's peers being the other clients.  Writes
        client<ID>_{balance,training,secagg}_input.json, the harness's file names, and prepared.json
        ({"clients": [{"id", "status", "root_D", "root_G", "root_W", "root_K", "gradient", "masked_update",
        "c1"}]}) into DIR; exit 0 when every client is OK, 1 when some client's gradient is above the
        clipping bound (status NORM; its files are still written and the witness engine refuses them),
        2 on a manifest of another shape or a value the library refuses (decided before the GPU is touched)

<circuit> is one of zkfl.circuits.CIRCUITS (poseidon_hash2, sgd_verified, sgd_step_v5,
balance_unified, secure_masked_update) followed by its integer template parameters.  GPU
commands use device $LOCAL_RANK (default 0).  Exit status 0 on success; verify and verify-round
exit 1 on an invalid proof, like snarkjs.
"""

from __future__ import annotations

import argparse
import json
import os
import secrets
import sys

from . import circuits, groth16, native, r1cs_file, snarkjs_cli, wprog, zkey


def _circuit(args):
    params = tuple(int(x) for x in args.params)
    b = circuits.build(args.circuit, *params)
    name = args.name or "_".join([args.circuit] + [str(p) for p in params])
    return b, name


def _ctx():
    return native.Context(int(os.environ.get("LOCAL_RANK", "0")))


def cmd_compile(args):
    b, name = _circuit(args)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, name + ".r1cs"), "wb") as f:
        f.write(b.r1cs_bytes())
    with open(os.path.join(args.out, name + ".zkwp"), "wb") as f:
        f.write(wprog.compile_program(b))
    if args.circom_layout:
        js = os.path.join(args.out, name + "_js")
        os.makedirs(js, exist_ok=True)
        with open(os.path.join(js, name + ".wasm"), "wb") as f:
            f.write(wprog.compile_program(b))
        gen = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "node", "generate_witness.cjs")
        with open(os.path.join(js, "generate_witness.cjs"), "w") as f:
            f.write("// written by `python -m zkfl compile --circom-layout`: circom's generate_witness.cjs over libzkfl\n"
                    f"require({json.dumps(gen)}).main(process.argv.slice(2));\n")
    print(f"template instances: {args.circuit}{tuple(args.params)}")
    print(f"non-linear constraints: {b.n_constraints}")
    print(f"wires: {b.n_wires}")
    print(f"written: {name}.r1cs, {name}.zkwp in {args.out}")


def _print_info(info):
    print(f"[INFO]  snarkJS: Curve: {info['curve']}")
    print(f"[INFO]  snarkJS: # of Wires: {info['wires']}")
    print(f"[INFO]  snarkJS: # of Constraints: {info['constraints']}")
    print(f"[INFO]  snarkJS: # of Private Inputs: {info['privateInputs']}")
    print(f"[INFO]  snarkJS: # of Public Inputs: {info['publicInputs']}")
    print(f"[INFO]  snarkJS: # of Labels: {info['labels']}")
    print(f"[INFO]  snarkJS: # of Outputs: {info['outputs']}")


def cmd_info(args):
    b, _ = _circuit(args)
    _print_info(groth16.r1cs_info(b))


def _read_r1cs(path):
    with open(path, "rb") as f:
        return r1cs_file.read_r1cs(f.read())


def cmd_r1cs_info(args):
    rc = _read_r1cs(args.r1cs)
    info = groth16.r1cs_info(rc)
    info["labels"] = rc.n_labels
    _print_info(info)


def _setup(b, name, out):
    os.makedirs(out, exist_ok=True)
    rnd = lambda: secrets.randbelow(zkey.R - 1) + 1  # noqa: E731
    with _ctx() as ctx:
        zk = zkey.groth16_setup(b, ctx, zkey.Toxic(tau=rnd(), alpha=rnd(), beta=rnd(), gamma=rnd(), delta=rnd()))
        vk = groth16.export_verification_key(zk, ctx=ctx)
    with open(os.path.join(out, name + "_final.zkey"), "wb") as f:
        f.write(zk)
    with open(os.path.join(out, "verification_key.json"), "w") as f:
        json.dump(vk, f, indent=1)
    print(f"written: {name}_final.zkey ({len(zk)} bytes), verification_key.json in {out}")


def cmd_setup_r1cs(args):
    name = args.name or os.path.splitext(os.path.basename(args.r1cs))[0]
    _setup(_read_r1cs(args.r1cs), name, args.out)


def cmd_setup(args):
    b, name = _circuit(args)
    _setup(b, name, args.out)


def cmd_export_vk(args):
    with _ctx() as ctx:
        vk = groth16.export_verification_key(open(args.zkey, "rb").read(), ctx=ctx)
    with open(args.vkey, "w") as f:
        json.dump(vk, f, indent=1)


def cmd_wtns(args):
    with _ctx() as ctx:
        wp = native.WitnessProgram(ctx, open(args.program, "rb").read())
        wt = wp.compute_json(open(args.input).read())
        wp.close()
    with open(args.out, "wb") as f:
        f.write(wt)


def cmd_prove(args):
    p = groth16.Prover(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        proof, public = p.prove(args.zkey, args.wtns, r1cs=args.r1cs, check_key=args.check_key)
    finally:
        p.close()
    with open(args.proof, "w") as f:
        json.dump(proof, f, indent=1)
    with open(args.public, "w") as f:
        json.dump(public, f, indent=1)


def cmd_verify(args):
    p = groth16.Prover(int(os.environ.get("LOCAL_RANK", "0")))
    ok = p.verify(json.load(open(args.vkey)), json.load(open(args.public)), json.load(open(args.proof)))
    p.close()
    if ok:
        print("[INFO]  snarkJS: OK!")
        return 0
    print("[ERROR] snarkJS: Invalid proof", file=sys.stderr)
    return 1


def _round_manifest(path):
    """round.json -> [(vkey path, public path, proof path)], or None with a message on stderr."""
    try:
        with open(path) as f:
            man = json.load(f)
    except (OSError, ValueError) as e:
        print(f"[ERROR] zkfl: {path}: {e}", file=sys.stderr)
        return None
    keys = ("vkey", "public", "proof")
    if not isinstance(man, list) or not all(
            isinstance(j, dict) and all(isinstance(j.get(k), str) for k in keys) for j in man):
        print(f"[ERROR] zkfl: {path}: expected a list of {{\"vkey\", \"public\", \"proof\"}} paths", file=sys.stderr)
        return None
    base = os.path.dirname(os.path.abspath(path))
    jobs = [tuple(os.path.join(base, j[k]) for k in keys) for j in man]
    for job in jobs:
        for f in job:
            if not os.path.isfile(f):
                print(f"[ERROR] zkfl: {path}: no such file: {f}", file=sys.stderr)
                return None
    return jobs


def cmd_verify_round(args):
    jobs = _round_manifest(args.round)
    if jobs is None:
        return 2
    try:
        data = [tuple(json.load(open(f)) for f in job) for job in jobs]
    except ValueError as e:
        print(f"[ERROR] zkfl: {args.round}: {e}", file=sys.stderr)
        return 2
    p = groth16.Prover(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        handles = {}
        for (vpath, _, _), (vk, _, _) in zip(jobs, data):
            if vpath not in handles:
                handles[vpath] = p.load_vkey(vk)
        round_jobs = [(handles[j[0]], d[1], d[2]) for j, d in zip(jobs, data)]
        if args.narrow:
            oks, rep = p.verify_round_narrow(round_jobs)
            print("[INFO]  zkfl: combined round, narrowed: " + ", ".join(f"{k} {v}" for k, v in rep.items()),
                  file=sys.stderr)
        elif args.combined:
            oks, rep = p.verify_round(round_jobs)
            print("[INFO]  zkfl: combined round: " + ", ".join(f"{k} {v}" for k, v in rep.items()), file=sys.stderr)
        else:
            oks = p.verify_multi(round_jobs)
    finally:
        p.close()
    for i, ok in enumerate(oks):
        print(f"job {i}: " + ("[INFO]  snarkJS: OK!" if ok else "[ERROR] snarkJS: Invalid proof"))
    return 0 if all(oks) else 1


def _aggregate_manifest(path):
    """round.json of `aggregate-round` -> (round, dim, groups for secagg.close_groups), or None with a
    message on stderr.  Everything that can be wrong with the manifest is decided here, on the host."""
    from . import secagg

    def bad(msg):
        print(f"[ERROR] zkfl: {path}: {msg}", file=sys.stderr)

    try:
        with open(path) as f:
            man = json.load(f)
    except (OSError, ValueError) as e:
        return bad(e)
    shape = ('expected {"round", "dim", "groups": [{"clients": [{"id", "accepted", "public"}], '
             '"revealed": [{"in", "out", "key"}]}]}')
    try:
        rnd, dim = int(man["round"]), int(man["dim"])
        if dim < 1 or not 0 <= rnd < zkey.R or not isinstance(man["groups"], list):
            return bad(shape)
        parsed = []
        for grp in man["groups"]:
            clients = [(int(c["id"]), bool(c["accepted"]), c.get("public")) for c in grp["clients"]]
            revealed = [(int(t["in"]), int(t["out"]), int(t["key"])) for t in grp["revealed"]]
            if any(acc and not isinstance(pub, str) for _, acc, pub in clients):
                return bad(shape)
            if not all(0 <= t[2] < zkey.R for t in revealed):
                return bad("a revealed key is not a field element")
            if not all(0 <= i < 1 << 64 for i in [c[0] for c in clients] + [x for t in revealed for x in t[:2]]):
                return bad("a client id is not an unsigned 64-bit integer")
            parsed.append((clients, revealed))
    except (KeyError, TypeError, ValueError, AttributeError):
        return bad(shape)
    base = os.path.dirname(os.path.abspath(path))
    groups = []
    for g, (clients, revealed) in enumerate(parsed):
        accepted = {}
        for cid, acc, pub in clients:
            if not acc:
                continue
            pub = os.path.join(base, pub)
            if not os.path.isfile(pub):
                return bad(f"no such file: {pub}")
            try:
                sig = [int(x) for x in json.load(open(pub))]
            except (OSError, ValueError, TypeError) as e:
                return bad(f"{pub}: {e}")
            # secure_masked_update's public signals: client_id, round, root_D, root_G, root_W, root_K,
            # tauSquared, masked_update[dim] (tests/full_system_simulation.mjs:999-1000)
            if len(sig) != 7 + dim:
                return bad(f"{pub}: expected {7 + dim} public signals, found {len(sig)}")
            if sig[0] != cid or sig[1] != rnd:
                return bad(f"{pub}: client_id {sig[0]}, round {sig[1]} where the manifest says client {cid}, round {rnd}")
            if cid in accepted:
                return bad(f"group {g}: client {cid} is listed twice")
            if not all(0 <= x < zkey.R for x in sig[7:7 + dim]):
                return bad(f"{pub}: a masked_update value is not a field element")
            accepted[cid] = sig[7:7 + dim]
        try:
            secagg.check_group(g, [c[0] for c in clients], list(accepted), revealed)
        except ValueError as e:
            return bad(e)
        groups.append({"roster": [c[0] for c in clients], "accepted": accepted, "revealed": revealed})
    return rnd, dim, groups


def cmd_aggregate_round(args):
    man = _aggregate_manifest(args.round)
    if man is None:
        return 2
    from . import secagg
    rnd, _, groups = man
    with _ctx() as ctx:
        sums = secagg.close_groups(ctx, groups, rnd)
    for g, s in enumerate(sums):
        line = {"group": g, "clients": s["clients"], "sum": s["sum"],
                "mean": None if s["sum"] is None else [x / s["clients"] for x in s["sum"]]}
        if s["out_of_range"]:
            line["out_of_range"] = True
        print(json.dumps(line))
    return 1 if any(s["out_of_range"] for s in sums) else 0


def _admit_manifest(path):
    """round.json of `admit-round` -> (the round dict of zkfl/admit.py, its packed arrays, the groups'
    rosters and revealed keys), or None with a message on stderr.  Host only."""
    from . import admit

    def bad(msg):
        print(f"[ERROR] zkfl: {path}: {msg}", file=sys.stderr)

    try:
        with open(path) as f:
            man = json.load(f)
    except (OSError, ValueError) as e:
        return bad(e)
    shape = ('expected {"round", "tau_squared", "dim", "vkeys": {"balance", "training", "secagg"}, '
             '"groups": [{"clients": [{"id", "balance", "training", "secagg"}]}]} (python -m zkfl --help)')
    base = os.path.dirname(os.path.abspath(path))

    def load(rel):
        if not isinstance(rel, str):
            raise ValueError(shape)
        full = os.path.join(base, rel)
        if not os.path.isfile(full):
            raise ValueError(f"no such file: {full}")
        try:
            with open(full) as f:
                return json.load(f)
        except ValueError as e:
            raise ValueError(f"{full}: {e}") from None

    try:
        if not isinstance(man, dict) or not isinstance(man["groups"], list):
            return bad(shape)
        rnd = {"round": man["round"], "tau_squared": man["tau_squared"], "dim": man["dim"], "clients": [],
               "vkeys": {p: load(man["vkeys"][p]) for p in admit.PHASES},
               "balance": {}, "training": {}, "secagg": {}, "peers": {}}
        if man.get("weights") is not None:
            rnd["weights"] = man["weights"]
        groups = []
        for grp in man["groups"]:
            roster = [int(c["id"]) for c in grp["clients"]]
            revealed = [(int(t["in"]), int(t["out"]), int(t["key"])) for t in grp.get("revealed", [])]
            if not all(0 <= t[2] < zkey.R for t in revealed):
                return bad("a revealed key is not a field element")
            for c in grp["clients"]:
                cid = int(c["id"])
                rnd["clients"].append(cid)
                rnd["peers"][cid] = c["peers"] if c.get("peers") is not None else [j for j in roster if j != cid]
                for p in admit.PHASES:
                    if c.get(p) is None:
                        continue
                    pkg = dict(c[p])
                    pkg["proof"], pkg["publicSignals"] = load(pkg.get("proof")), load(pkg.pop("public", None))
                    rnd[p][cid] = pkg
            groups.append((roster, revealed))
        packed = admit.pack(rnd)
        for p in admit.PHASES:
            groth16.vk_bytes(rnd["vkeys"][p])
    except ValueError as e:
        return bad(e)
    except (KeyError, TypeError, AttributeError, AssertionError):
        return bad(shape)
    return rnd, packed, groups


def cmd_admit_round(args):
    man = _admit_manifest(args.round)
    if man is None:
        return 2
    from . import admit, secagg
    rnd, packed, groups = man
    p = groth16.Prover(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        res = admit.admit_round(p, rnd, reference=args.reference, combined=args.combined, packed=packed)
        if args.combined:
            print("[INFO]  zkfl: combined round: " + ", ".join(f"{k} {v}" for k, v in res.report.items()),
                  file=sys.stderr)
        for cid, names in res.names.items():
            for phase, name in zip(admit.PHASES, names):
                print(f"client {cid} {phase}: {name}")
        rc = 0 if all(c == 0 or native.ADMIT_CODES[c].endswith("_MISSING")
                      for cs in res.codes.values() for c in cs) else 1
        if args.aggregate:
            dim, ok = int(rnd["dim"]), set(res.accepted)
            todo = []
            for g, (roster, revealed) in enumerate(groups):
                acc = {c: [int(x) for x in rnd["secagg"][c]["publicSignals"][7:7 + dim]] for c in roster if c in ok}
                if acc:
                    todo.append((g, {"roster": roster, "accepted": acc, "revealed": revealed}))
            try:
                sums = dict(zip((g for g, _ in todo),
                                secagg.close_groups(p.ctx, [grp for _, grp in todo], int(rnd["round"]))))
            except ValueError as e:
                print(f"[ERROR] zkfl: {args.round}: {e}", file=sys.stderr)
                return 1
            for g in range(len(groups)):
                s = sums.get(g)
                line = {"group": g, "clients": s["clients"] if s else 0, "sum": s["sum"] if s else None,
                        "mean": None if not s or s["sum"] is None else [x / s["clients"] for x in s["sum"]]}
                if s and s["out_of_range"]:
                    line["out_of_range"] = True
                    rc = 1
                print(json.dumps(line))
    finally:
        p.close()
    return rc


def _prepare_manifest(path):
    """manifest.json of `prepare-round` -> the packed spec of zkfl/prepare.py, or None with a message on
    stderr.  Host only."""
    from . import prepare

    def bad(msg):
        print(f"[ERROR] zkfl: {path}: {msg}", file=sys.stderr)

    shape = ('expected {"round", "tau_squared", "depth", "batch", "precision", "weights", "clients": [{"id", '
             '"features", "labels"}]} (python -m zkfl --help)')
    try:
        with open(path) as f:
            man = json.load(f)
    except (OSError, ValueError) as e:
        return bad(e)
    try:
        if not isinstance(man, dict) or not isinstance(man["clients"], list) or not man["clients"]:
            return bad(shape)
        cl = man["clients"]
        ids = [int(c["id"]) for c in cl]
        feats = [c["features"] for c in cl]
        spec = {"ids": ids, "samples": len(feats[0]), "dim": len(man["weights"]), "depth": man["depth"],
                "batch": man["batch"], "precision": man["precision"], "weights": man["weights"],
                "round": man["round"], "tau_squared": man["tau_squared"], "features": feats,
                "labels": [c["labels"] for c in cl]}
        if any(c.get("batch_idx") is not None for c in cl):
            spec["batch_idx"] = [c["batch_idx"] for c in cl]
        if man.get("harness_keys"):
            spec["peers"], spec["keys"], spec["master_keys"] = prepare.harness_keys(ids)
        elif any(c.get("peers") is not None for c in cl):
            spec["peers"] = [c["peers"] for c in cl]
            spec["keys"] = [c["keys"] for c in cl]
            spec["master_keys"] = [c["master_key"] for c in cl]
        return prepare.pack(spec)
    except ValueError as e:
        return bad(e)
    except (KeyError, TypeError, AttributeError, IndexError):
        return bad(shape)


def cmd_prepare_round(args):
    packed = _prepare_manifest(args.manifest)
    if packed is None:
        return 2
    from . import prepare
    with _ctx() as ctx:
        res = prepare.prepare_round(ctx, None, packed=packed)
    os.makedirs(args.out, exist_ok=True)
    summary = []
    for i, cid in enumerate(res.ids):
        for phase in res.inputs:
            with open(os.path.join(args.out, f"client{cid}_{phase}_input.json"), "w") as f:
                json.dump(res.input_json(phase, i), f)
        d, g, w, k = (str(x) for x in prepare._ints(res.roots[i]))
        summary.append({"id": cid, "status": prepare.STATUS[int(res.status[i])], "root_D": d, "root_G": g, "root_W": w,
                        "root_K": k if packed["peers"] else None, "gradient": [int(x) for x in res.gradients[i]],
                        "masked_update": [str(x) for x in prepare._ints(res.masked[i])] if res.masked is not None else None,
                        "c1": int(res.c1[i])})
        print(f"client {cid}: {summary[-1]['status']}")
    with open(os.path.join(args.out, "prepared.json"), "w") as f:
        json.dump({"round": str(packed["round"]), "tau_squared": str(packed["tau_squared"]), "clients": summary}, f)
    return 0 if res.ok else 1


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if snarkjs_cli.routes(argv):   # snarkjs ceremony strings and `wtns check` (zkfl/snarkjs_cli.py)
        return snarkjs_cli.run(argv)
    ap = argparse.ArgumentParser(prog="python -m zkfl", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)

    def circuit_args(sp, out=False):
        sp.add_argument("circuit", choices=sorted(circuits.CIRCUITS))
        sp.add_argument("params", nargs="*")
        sp.add_argument("--name", default=None, help="output base name (default: circuit_params)")
        if out:
            sp.add_argument("-o", "--out", default=".")

    sp = sub.add_parser("compile")
    circuit_args(sp, out=True)
    sp.add_argument("--circom-layout", action="store_true",
                    help="also write <name>_js/<name>.wasm + generate_witness.cjs (circom's output layout)")
    circuit_args(sub.add_parser("info"))
    circuit_args(sub.add_parser("setup"), out=True)
    sp = sub.add_parser("r1cs-info")
    sp.add_argument("r1cs")
    sp = sub.add_parser("setup-r1cs")
    sp.add_argument("r1cs")
    sp.add_argument("--name", default=None, help="output base name (default: the .r1cs file's)")
    sp.add_argument("-o", "--out", default=".")
    sp = sub.add_parser("export-vk")
    sp.add_argument("zkey")
    sp.add_argument("vkey")
    sp = sub.add_parser("wtns")
    sp.add_argument("program")
    sp.add_argument("input")
    sp.add_argument("out")
    sp = sub.add_parser("prove")
    for a in ("zkey", "wtns", "proof", "public"):
        sp.add_argument(a)
    sp.add_argument("--r1cs", default=None, help="check the witness against this .r1cs before proving")
    sp.add_argument("--check-key", nargs=2, default=None, metavar=("R1CS", "PTAU"),
                    help="check the key against this .r1cs and prepared .ptau before loading it")
    sp = sub.add_parser("verify")
    for a in ("vkey", "public", "proof"):
        sp.add_argument(a)
    sp = sub.add_parser("verify-round")
    sp.add_argument("round")
    sp.add_argument("--combined", action="store_true",
                    help="one random combination and one final exponentiation for the whole round")
    sp.add_argument("--narrow", action="store_true",
                    help="--combined, and a failed round is narrowed to its bad groups before the per-proof path")
    sp = sub.add_parser("aggregate-round")
    sp.add_argument("round")
    sp = sub.add_parser("admit-round")
    sp.add_argument("round")
    sp.add_argument("--reference", action="store_true", help="only the reference server's checks")
    sp.add_argument("--combined", action="store_true",
                    help="one random combination and one final exponentiation for the round's proofs")
    sp.add_argument("--aggregate", action="store_true",
                    help="then aggregate each group over its accepted clients (aggregate-round's lines)")
    sp = sub.add_parser("prepare-round")
    sp.add_argument("manifest")
    sp.add_argument("-o", "--out", required=True, help="the directory the input.json files go to")
    args = ap.parse_args(argv)
    fn = {"compile": cmd_compile, "info": cmd_info, "setup": cmd_setup,
          "r1cs-info": cmd_r1cs_info, "setup-r1cs": cmd_setup_r1cs, "export-vk": cmd_export_vk,
          "wtns": cmd_wtns, "prove": cmd_prove, "verify": cmd_verify, "verify-round": cmd_verify_round,
          "aggregate-round": cmd_aggregate_round, "admit-round": cmd_admit_round,
          "prepare-round": cmd_prepare_round}[args.cmd]
    try:
        return fn(args) or 0
    except native.ZkflError as e:
        print(f"[ERROR] zkfl: {e}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
