"""Leiden communities of the pooled cells on the MI355X: Louvain's move phase, a refinement of every community into connected parts
and aggregation by the parts, on the integer level graphs of jamie_amd/louvain.py.  O(nnz) memory.

    level_record(...)                                  the record of a level: Louvain's, and refined, merged, cancelled
    start(G)                                           every node alone: ref, rtot, rsize (and the cut table, the targets, the counts)
    cut_table(G, comm, R), refine, apply               one class's sub-sweep: the cut of every part, the targets, their application
    refine_level(G, state, R, gamma)                   the 8 sub-sweeps of a level's refinement; (merged, cancelled)
    next_partition(comm, cmap, nc)                     the start partition of the next level: the lowest part of every community
    communities(graph), leiden(embeddings, labels)     the whole run on a `FuzzyGraph`; JAMIE.leiden on the device

The kernels are in csrc/leiden.hip (include/jamie_hip.h, "Leiden communities on the device").  The graph, the level graph, a sweep,
the move phase (`run_level` from a partition), the aggregation, the tables of Q, the summary and the pooled front end are louvain.py's.  The definition (shared with the int64 / float64 host route of
jamie.py) is DESIGN.md §24: every sum of weights is an int64 sum, so the device route equals a numpy restatement element for
element and run for run, and every returned community is connected unless the run stopped at max_levels.
"""
import torch

from . import _native as nv
from . import louvain as jlv

STOPS = ('singletons', 'stuck', 'max_levels')


def level_record(nodes, communities, history, modularity, two_m, refined=None, merged=None, cancelled=None):
    """Louvain's record of a level and the figures of its refinement: `refined` the parts (the next level's nodes), `merged` the
    nodes that joined a part, `cancelled` the joins refused because the part's founder was itself leaving.  Each None on the last
    level of a run that ended 'singletons' or 'max_levels', where nothing is refined."""
    rec = jlv.level_record(nodes, communities, history, modularity, two_m)
    rec.update(refined=None if refined is None else int(refined), merged=None if merged is None else int(merged),
               cancelled=None if cancelled is None else int(cancelled))
    return rec


class Refinement:
    """ref int32 [n], rtot int64 [n], rsize int32 [n] of a level's refinement on the device, the cut table, the targets of the
    last `refine` and the (merged, cancelled) counts."""

    def __init__(self, ref, rtot, rsize):
        dev = ref.device
        self.ref, self.rtot, self.rsize = ref, rtot, rsize
        self.cut = torch.zeros_like(rtot)
        self.target = ref.clone()
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)


def start(G):
    dev = G.col.device
    return Refinement(torch.arange(G.n, dtype=torch.int32, device=dev), G.k.clone(), torch.ones(G.n, dtype=torch.int32, device=dev))


def refinement_of(G, ref):
    """The refinement state of the parts `ref` (numpy or tensor; a part is named after a member): rtot and rsize by integer sums."""
    st = jlv.state_of(G, ref)
    return Refinement(st.comm, st.tot, st.size)


def cut_table(G, comm, R):
    """R.cut[s] = the weights of the stored entries that leave part s inside its community, from scratch."""
    nv.require_gpu()
    nv.leiden_cut(G.rowptr, G.col, G.w, comm, R.ref, R.cut)


def refine(G, state, R, cls, gamma=1.0):
    """The targets of the nodes of class `cls` from the state as it stands, into R.target (the other classes' entries are left
    alone); the (short, long, global) row counts the launch took."""
    nv.require_gpu()
    nodes, counts, slot_off, ws = G.of_class(cls)
    if sum(counts):
        nv.leiden_refine(G.rowptr, G.col, G.w, G.k, state.comm, state.tot, R.ref, R.rtot, R.rsize, R.cut, float(gamma), G.two_m,
                         nodes, counts, slot_off, ws, R.target, R.flag)
    return counts


def apply(G, R, cls):
    """Applies R.target to the nodes of class `cls`: ref, rtot, rsize by integer atomics; R.counts grows by the merged and the
    cancelled moves."""
    nv.require_gpu()
    nodes = G.of_class(cls)[0]
    if nodes.numel():
        nv.leiden_apply(nodes, R.target, G.k, R.ref, R.rtot, R.rsize, R.counts)


def refine_level(G, state, R, gamma=1.0, trace=None):
    """The 8 sub-sweeps of DESIGN.md §24 step 3 on the communities of `state`: a fresh copy of ref as the targets, the cut table,
    the proposals of the class, their application.  (merged, cancelled).  `trace` (a list) receives, per sub-sweep, ref and cut as
    numpy arrays and the two counts so far."""
    R.counts.zero_()
    for s in range(jlv.CLASSES):
        R.target.copy_(R.ref)
        cut_table(G, state.comm, R)
        refine(G, state, R, s, gamma)
        apply(G, R, s)
        if trace is not None:
            merged, cancelled = (int(v) for v in R.counts.tolist())
            trace.append(dict(ref=R.ref.cpu().numpy().astype('int64'), cut=R.cut.cpu().numpy(), merged=merged, cancelled=cancelled))
    if int(R.flag.item()):
        raise RuntimeError('leiden: a row did not fit the bin its node list put it in')
    merged, cancelled = (int(v) for v in R.counts.tolist())
    return merged, cancelled


def next_partition(comm, cmap, nc):
    """comm0 int32 [nc] of the next level: every part r starts in the lowest coarse id among the parts of its community.  Integer
    `scatter_reduce` (amin) and a scatter of equal values."""
    c = comm.long()
    low = torch.full((comm.numel(),), nc, dtype=torch.int64, device=comm.device).scatter_reduce_(0, c, cmap, 'amin')
    comm0 = torch.empty(nc, dtype=torch.int64, device=comm.device)
    comm0[cmap] = low[c]                                   # (the members of a part share a community: equal values)
    return comm0.to(torch.int32)


def communities_of_level_graph(G, resolution=1.0, max_levels=20, max_sweeps=32, trace=None):
    """The run of DESIGN.md §24 on an integer level graph: dict(comm int64 numpy [n]: the returned partition composed down to the
    level-0 nodes, modularity, levels, stop).  `trace` (a list) receives one list per refined level (`refine_level`)."""
    jlv.check_totals(G.n, G.two_m, 'leiden')
    two_m = G.two_m
    cells = torch.arange(G.n, dtype=torch.int64, device=G.col.device)
    comm0, levels = None, []
    while True:
        state, history = jlv.run_level(G, resolution, max_sweeps, comm0)      # the move phase: DESIGN.md §23 steps 2-3
        inside = jlv.internal_weights(G, state.comm)
        q = jlv.modularity_from_tables(inside.cpu().numpy(), state.tot.cpu().numpy(), two_m, resolution)
        nc = int((state.size > 0).sum().item())
        if nc == G.n or len(levels) + 1 >= max_levels:
            levels.append(level_record(G.n, nc, history, q, two_m))
            stop = 'singletons' if nc == G.n else 'max_levels'
            return dict(comm=state.comm.long()[cells].cpu().numpy(), modularity=q, levels=levels, stop=stop)
        R = start(G)
        sub = None
        if trace is not None:
            sub = []
            trace.append(sub)
        merged, cancelled = refine_level(G, state, R, resolution, sub)
        if merged == 0:
            levels.append(level_record(G.n, nc, history, q, two_m, G.n, 0, cancelled))
            q = jlv.modularity_from_tables(G.loop.cpu().numpy(), G.k.cpu().numpy(), two_m, resolution)
            return dict(comm=cells.cpu().numpy(), modularity=q, levels=levels, stop='stuck')
        nxt, cmap = jlv.aggregate(G, R.ref)
        levels.append(level_record(G.n, nc, history, q, two_m, nxt.n, merged, cancelled))
        comm0 = next_partition(state.comm, cmap, nxt.n)
        cells = cmap[cells]
        G = nxt


def communities(graph, resolution=1.0, max_levels=20, max_sweeps=32, tol=1e-7, trace=None):
    """Leiden communities of a `FuzzyGraph`: dict(clusters int32 [N], sizes, modularity, levels, stop).  `tol` is accepted for
    parity with `louvain.communities` and unused.  Bit-identical from run to run."""
    out = communities_of_level_graph(jlv.level_graph(graph), resolution, max_levels, max_sweeps, trace)
    clusters, sizes = jlv.relabel(out['comm'])
    return dict(clusters=clusters, sizes=sizes, modularity=out['modularity'], levels=out['levels'], stop=out['stop'])


def leiden_summary(out, *rest):
    """`louvain_summary`'s dict and `stop`."""
    res = jlv.run_summary(out, *rest)
    res['stop'] = out['stop']
    return res


def leiden(embeddings, labels=None, resolution=1.0, n_neighbors=15, max_levels=20, max_sweeps=32, tol=1e-7, return_graph=False,
           device='cuda'):
    """Leiden communities of M embeddings [N_m, L] pooled into one set of cells: the dict of `louvain.louvain`, with

        levels                      per level: nodes, communities, sweeps, moved (per sweep), modularity, refined, merged,
                                    cancelled, two_m
        stop                        'singletons' | 'stuck' | 'max_levels'

    Every community is connected in the graph unless stop is 'max_levels'.  `tol` is accepted for parity with `louvain` and
    unused.  Bit-identical from run to run."""
    checked = jlv.check_louvain(embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, 'leiden')
    return leiden_checked(embeddings, labels, *checked, return_graph, device)


def leiden_checked(embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps, tol, return_graph=False, device='cuda'):
    """`leiden` behind its argument checks: the arguments are what `check_louvain` returned."""
    return jlv.pooled_run('leiden', communities, leiden_summary, embeddings, labels, resolution, n_neighbors, max_levels, max_sweeps,
                          tol, return_graph, device)
