"""Regenerate tests/golden/route_labels.json: which kernels the colour render step took, as svox_t_amd.csrc.LAST_ROUTE
names them, and which entry points of the library the host called for it, recorded on the GPU from the code that is
checked out -- the file that is committed was written by the commit BEFORE the host's routes became records
("One route record for the render step"), so that the records are held to what the interleaved code did:

    python tests/golden/make_route_golden.py --commit <the revision that is checked out>

One entry per (payload, batch, route, fast) that tests/test_gpu_route_matrix.py::routes yields for the trees of seed 0 --
the step itself, the second backward of the default route, the forward under no_grad with the route's switches -- plus,
per payload and batch, render_persp (image batches without view rotations) and the no_grad forward with scratch lists of
4 records.  Nothing is asserted and no switch is set that the route matrix does not set.  Labels and call sequences repeat
heavily: the file keeps the distinct strings, the distinct call sequences and the distinct outcomes once and an entry is
four small numbers.  tests/test_route_host.py reproduces every entry without a GPU."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "route_labels.json")
SEED = 0
PERSP, SCRATCH4 = "render_persp", "FWD_LIST_SAMPLES=4 no_grad"        # the two walks of the matrix that are no route
# an outcome: the step's forward, its backward, the default route's second backward, the forward under no_grad
FIELDS = ("forward", "forward_terms", "forward_calls", "backward", "backward_calls", "second_backward", "second_backward_calls",
          "no_grad_forward", "no_grad_calls")


class Table:
    """Distinct values in the order they were first seen."""

    def __init__(self):
        self.values, self.index = [], {}

    def __call__(self, v):
        if v is None:
            return None
        if v not in self.index:
            self.index[v] = len(self.values)
            self.values.append(v)
        return self.index[v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown", help="the revision that is checked out (kept in the file)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch

    import svox_t_amd.csrc as _C
    from tests import test_gpu_route_matrix as G
    from tests import test_route_matrix_host as H

    gpu = torch.device("cuda:0")
    called = []
    real_call = _C._call

    def spy(name, *a):
        called.append(name)
        return real_call(name, *a)
    _C._call = spy

    class switches:
        def __init__(self, sw):
            self.sw, self.old = sw, []

        def __enter__(self):
            for k, v in self.sw.items():
                if k == "_again":
                    continue
                k, v = ("_pool_blocks_for", lambda tiles, S, kind="record": 32) if k == "_dry" else (k, v)
                self.old.append((k, getattr(_C, k)))
                setattr(_C, k, v)

        def __exit__(self, *exc):
            for k, v in reversed(self.old):
                setattr(_C, k, v)
            return False

    labels, calls, outcomes, payloads, batches, names = Table(), Table(), Table(), Table(), Table(), Table()

    def forward(g, f, fast, persp=False, **kw):
        del called[:]
        out = g.forward(f, fast, persp, **kw)
        return out, [labels(_C.LAST_ROUTE["forward"]), bool(_C.LAST_ROUTE["forward_terms"]), calls(tuple(called))]

    def step(g, fast, backwards, persp=False, **kw):
        f = g.f.detach().clone().requires_grad_(True)
        out, got = forward(g, f, fast, persp, **kw)
        for i in range(2):
            if i < backwards:
                del called[:]
                torch.autograd.grad(out, f, g.g, retain_graph=i + 1 < backwards)
                got += [labels(_C.LAST_ROUTE["backward"]), calls(tuple(called))]
            else:
                got += [None, None]
        return got

    def no_grad(g, fast, **kw):
        with torch.no_grad():
            _, got = forward(g, g.f, fast, **kw)
        return [got[0], got[2]]

    entries = []
    for payload in H.PAYLOADS:
        for batch in H.BATCHES:
            a = H.inputs(payload, SEED, batch)
            g = G.OnGpu(a, gpu)
            for name, sw, kw in G.routes(a):
                with switches(sw):
                    for fast in (False, True):
                        o = step(g, fast, 2 if name == "default" else 1, **kw) + no_grad(g, fast, **kw)
                        entries.append([payloads(payload), batches(batch), names(name), int(fast), outcomes(tuple(o))])
            with switches({"FWD_LIST_SAMPLES": 4}):
                for fast in (False, True):
                    o = [None] * 7 + no_grad(g, fast)
                    entries.append([payloads(payload), batches(batch), names(SCRATCH4), int(fast), outcomes(tuple(o))])
            if a.image is not None and a.xf is None:
                for fast in (False, True):
                    o = step(g, fast, 1, persp=True) + [None, None]
                    entries.append([payloads(payload), batches(batch), names(PERSP), int(fast), outcomes(tuple(o))])
            torch.cuda.synchronize()
            print(f"{payload}/{SEED}/{batch}: {len(entries)} entries, {len(outcomes.values)} outcomes, {len(labels.values)} labels",
                  flush=True)
    doc = [("recorded_from", args.commit), ("seed", SEED), ("fields_of_an_outcome", list(FIELDS)), ("count", len(entries)),
           ("labels", labels.values), ("calls", [list(c) for c in calls.values]), ("payloads", payloads.values),
           ("batches", batches.values), ("routes", names.values), ("outcomes", [list(o) for o in outcomes.values])]
    write(args.out, doc, entries)
    print(f"{len(entries)} entries, {len(outcomes.values)} outcomes, {len(labels.values)} labels -> {args.out}")


def write(path, doc, entries):
    """entries [payload, batch, route, fast, outcome], fast False then True per route, as walks: one per payload and batch,
    [payload, batch, route list, outcomes at thresholds 0, outcomes fast]; the distinct route lists are kept once."""
    lists, walks = Table(), []
    for p, b, r, fast, o in entries:
        if not walks or walks[-1][:2] != [p, b]:
            walks.append([p, b, [], [], []])
        if not fast:
            walks[-1][2].append(r)
        assert walks[-1][2][-1] == r and len(walks[-1][3 + fast]) == len(walks[-1][2]) - 1
        walks[-1][3 + fast].append(o)
    for w in walks:
        w[2] = lists(tuple(w[2]))
    doc = doc + [("fields_of_a_walk", ["payload", "batch", "route list", "outcome per route", "outcome per route, fast"]),
                 ("route_lists", [list(x) for x in lists.values]), ("walks", walks)]
    rows = ("labels", "calls", "outcomes", "route_lists", "walks")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: " + (json.dumps(v, separators=(",", ":")) if k not in rows else
                                                           "[\n" + ",\n".join("  " + json.dumps(x, separators=(",", ":")) for x in v)
                                                           + "\n ]") for k, v in doc) + "\n}\n")


def read(path=OUT):
    """(the file, [(payload, batch, route, fast, {field: label / call names / flag, or None})]): every entry spelt out."""
    with open(path) as f:
        d = json.load(f)
    entries = []
    for p, b, rl, slow, fast in d["walks"]:
        for i, r in enumerate(d["route_lists"][rl]):
            for fl, o in ((False, slow[i]), (True, fast[i])):
                out = {}
                for name, v in zip(d["fields_of_an_outcome"], d["outcomes"][o]):
                    out[name] = None if v is None else d["calls"][v] if name.endswith("calls") else \
                        v if name == "forward_terms" else d["labels"][v]
                entries.append((d["payloads"][p], d["batches"][b], d["routes"][r], fl, out))
    return d, entries


if __name__ == "__main__":
    main()
