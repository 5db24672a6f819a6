#!/usr/bin/env python
"""Generate tests/golden/g14_distortion_{reference,lorentz}.{npz,json} by running the REFERENCE's
``scripts/eval_hierarchy.py`` (``set_seeds``, ``create_node_mapping``, ``compute_distortion``) on the CPU.

Like its siblings it runs only where the reference is present (it is executed, never copied) and applies the sign patch of
make_golden.py to ``embedding.lorentz_model.minkowski_dot``:
  reference : the module exactly as shipped (every distance is 0.0, so every ratio is 0.0)
  lorentz   : ``minkowski_dot`` negated
While the reference runs, ``nx.shortest_path_length`` is replaced by a spy that records every (a, b) it is asked for and the
length it answers (-1 where it raises ``NetworkXNoPath``): that is the sequence of ``random.sample`` draws, retries included.

The json holds every graph once under ``graphs`` (the node names in ``.nodes()`` order, the vocabulary, the reference's
mapping as an ordered list of [node, index]) and per case: its graph's name, seed, curvature, ``num_pairs``, the
reference's statistics, the number of distinct first nodes among the accepted pairs, and the sha256 of
``repr(random.getstate())`` after the run.  The npz holds per graph ``<graph>__edges`` int32 [E, 2] (node positions) and
``<graph>__emb`` fp32 [V, d + 1], per case ``<name>__tried`` int32 [T, 3] (a, b, length or -1) and ``<name>__ratios`` float64.

Cases (graphs of a few hundred nodes at most, d = 8):
  tree_s1, tree_s63, tree_s64, tree_s65, tree_s130   a random tree of 300 nodes; num_pairs is the smallest count that gives
                                    that many distinct sources (1, below / at / above one 64-bit word, three words)
  cycles     a tree of 200 nodes plus 80 chords
  forest     three components, an isolated node and a self-loop: the sampler retries
  synsets    names ``word.n.0k``: two nodes share a word (one vocabulary index), some words are missing from the
             vocabulary, one token occurs twice in it (the first index counts)
  path70     a path of 70 nodes: more than 64 levels deep
  star100    a centre with 100 leaves: a degree above the wave size

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distortion.py [reference|lorentz|all]
"""
from __future__ import annotations

import json
import logging
import os
import random
import sys
import types
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_distortion.py: /root/reference is not present; golden vectors can only be regenerated "
             "in the build container.")

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import embedding.lorentz_model as L  # noqa: E402  (reference)

import hierarchy_cases as HC  # noqa: E402  (ours: the pure-Python truth the generator checks itself against)

_ORIG = L.minkowski_dot
D, SEED, CURVATURE = 8, 42, 1.0


def set_mode(mode: str) -> None:
    if mode == "reference":
        L.minkowski_dot = _ORIG
    elif mode == "lorentz":
        L.minkowski_dot = lambda a, b: -_ORIG(a, b)
    else:
        raise ValueError(mode)


def load_script():
    path = os.path.join(REF, "scripts", "eval_hierarchy.py")
    mod = types.ModuleType("reference_eval_hierarchy")
    mod.__file__ = path
    exec(compile(open(path).read(), path, "exec"), mod.__dict__)
    logging.getLogger().setLevel(logging.ERROR)
    mod.logger.setLevel(logging.ERROR)
    return mod


# ---- graphs: (node names, edges as positions) ---------------------------------------------------------------------------
def random_tree(rs, n):
    return [(int(rs.randint(0, k)), k) for k in range(1, n)]


def plain_names(rs, n):
    names = [f"n{k}" for k in range(n)]
    rs.shuffle(names)
    return names


def g_tree(rs):
    return plain_names(rs, 300), random_tree(rs, 300)


def g_cycles(rs):
    edges = random_tree(rs, 200)
    edges += [(int(a), int(b)) for a, b in rs.randint(0, 200, (80, 2))]
    return plain_names(rs, 200), edges


def g_forest(rs):
    edges, base = [], 0
    for size in (60, 40, 25):
        edges += [(base + a, base + b) for a, b in random_tree(rs, size)]
        base += size
    edges.append((7, 7))                                   # a self-loop; node `base` (the last one) has no edge at all
    perm = rs.permutation(base + 1)                        # components interleaved in index order
    return plain_names(rs, base + 1), [(int(perm[a]), int(perm[b])) for a, b in edges]


def g_synsets(rs):
    n = 150
    words = [f"w{k // 2}" if k < 60 else f"w{k}" for k in range(n)]        # the first 60 nodes share 30 words
    names = [f"{w}.n.0{1 + (k % 2 if k < 60 else 0)}" for k, w in enumerate(words)]
    edges = random_tree(rs, n) + [(int(a), int(b)) for a, b in rs.randint(0, n, (20, 2))]
    return names, edges


def g_path(rs):
    return plain_names(rs, 70), [(k, k + 1) for k in range(69)]


def g_star(rs):
    return plain_names(rs, 101), [(0, k) for k in range(1, 101)]


def vocab_for(rs, names, synsets):
    words = list(dict.fromkeys(nm.split(".")[0] for nm in names))
    rs.shuffle(words)
    if synsets:
        words = words[: len(words) - 25]                   # 25 words are missing from the vocabulary
        words = words + [words[3], words[10]]              # tokens that occur twice: the first index counts
    return ["<pad>", "<unk>"] + words


def embeddings_for(rs, v):
    x = rs.randn(v, D + 1).astype(np.float32) * np.float32(0.8)
    x[:, 0] = np.sqrt(np.float32(1.0) + (x[:, 1:] * x[:, 1:]).sum(-1, dtype=np.float32))
    return x


#: (name, graph builder, synset-style vocabulary, num_pairs or None, distinct sources wanted or None)
CASES = (
    ("tree_s1", g_tree, False, None, 1),
    ("tree_s63", g_tree, False, None, 63),
    ("tree_s64", g_tree, False, None, 64),
    ("tree_s65", g_tree, False, None, 65),
    ("tree_s130", g_tree, False, None, 130),
    ("cycles", g_cycles, False, 40, None),
    ("forest", g_forest, False, 60, None),
    ("synsets", g_synsets, True, 50, None),
    ("path70", g_path, False, 30, None),
    ("star100", g_star, False, 30, None),
)


def run_reference(script, graph, vocab, emb, num_pairs):
    tried = []
    real = nx.shortest_path_length

    def spy(g, a, b, *args, **kw):
        try:
            length = real(g, a, b, *args, **kw)
        except nx.NetworkXNoPath:
            tried.append((a, b, -1))
            raise
        tried.append((a, b, int(length)))
        return length

    nx.shortest_path_length = spy
    try:
        script.set_seeds(SEED)
        mapping = script.create_node_mapping(graph, vocab)
        ratios, stats = script.compute_distortion(graph, torch.from_numpy(emb), mapping, num_pairs=num_pairs,
                                                  curvature=CURVATURE, device=torch.device("cpu"))
        state = HC.rng_hash()
    finally:
        nx.shortest_path_length = real
    return mapping, tried, np.asarray(ratios, np.float64), stats, state


def generate(mode: str) -> None:
    set_mode(mode)
    script = load_script()
    arrays, cases, graphs = {}, [], {}
    for name, build, synsets, num_pairs, want_sources in CASES:
        rs = np.random.RandomState(sum(build.__name__.encode()) + 1000)      # the same graph for every run on it
        names, edges = build(rs)
        vocab = vocab_for(rs, names, synsets)
        emb = embeddings_for(rs, len(vocab))
        graph = nx.Graph()
        graph.add_nodes_from(names)
        graph.add_edges_from((names[a], names[b]) for a, b in edges)
        assert list(graph.nodes()) == names
        index = {nm: k for k, nm in enumerate(names)}
        if want_sources is not None:                       # the sampler is sequential: a shorter run is a prefix of a longer one
            _, tried, _, _, _ = run_reference(script, graph, vocab, emb, 600)
            seen, num_pairs = set(), None
            for k, (a, _, _) in enumerate(t for t in tried if t[2] >= 0):
                seen.add(a)
                if len(seen) == want_sources:
                    num_pairs = k + 1
                    break
            assert num_pairs is not None, name
        mapping, tried, ratios, stats, state = run_reference(script, graph, vocab, emb, num_pairs)
        accepted = [t for t in tried if t[2] >= 0]
        assert len(accepted) == num_pairs == len(ratios)
        sources = len({a for a, _, _ in accepted})
        assert want_sources is None or sources == want_sources, (name, sources)
        # the generator's own check: the pure-Python truth of the tests agrees with networkx on every answer
        adj = HC.adjacency(len(names), edges)
        labels = HC.component_labels(len(names), edges)
        for a, b, length in tried:
            assert HC.bfs_lengths(adj, index[a])[index[b]] == length, (name, a, b)
            assert (labels[index[a]] == labels[index[b]]) == (length >= 0)
        if name == "forest":
            assert any(t[2] < 0 for t in tried), "the forest case must make the sampler retry"
        if name == "path70":
            assert max(t[2] for t in tried) > 40
        if synsets:
            assert len(set(mapping.values())) < len(mapping) < len(names)
        gname = build.__name__[2:]
        entry = {"nodes": names, "vocab": vocab, "mapping": [[k, int(v)] for k, v in mapping.items()]}
        assert graphs.setdefault(gname, entry) == entry, name                  # every run on a graph sees the same inputs
        arrays[f"{gname}__edges"] = np.array(edges, np.int32).reshape(-1, 2)
        arrays[f"{gname}__emb"] = emb
        arrays[f"{name}__tried"] = np.array([(index[a], index[b], ln) for a, b, ln in tried], np.int32).reshape(-1, 3)
        arrays[f"{name}__ratios"] = ratios
        cases.append({"name": name, "graph": gname, "seed": SEED, "curvature": CURVATURE, "num_pairs": num_pairs,
                      "stats": stats, "distinct_sources": sources,
                      "retries": len(tried) - len(accepted), "rng_hash": state})
        print(f"{mode}: {name}: pairs {num_pairs} sources {sources} retries {len(tried) - len(accepted)} mean {stats['mean']:.6g}", flush=True)
    np.savez_compressed(os.path.join(HERE, f"g14_distortion_{mode}.npz"), **arrays)
    with open(os.path.join(HERE, f"g14_distortion_{mode}.json"), "w") as f:
        json.dump({"mode": mode, "d": D, "graphs": graphs, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for m in (("reference", "lorentz") if which == "all" else (which,)):
        generate(m)
