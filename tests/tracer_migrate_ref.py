"""numpy restatement of the migration of tracer particles between ranks (castro_amd/csrc/tracer_kernels.hip: k_tracer_dest,
k_tracer_scan, k_tracer_pack, k_tracer_unpack; include/castro_hydro_amd.h): the destination of every particle and the counts, the
stable partition into kept arrays and wire records, and the unpack.  Integer work and bit copies: compared bit for bit.
Tests only.

Particles: the dict of tests/tracer_ref.py.  level_owners[l][g]: the rank that owns box g of level l.
Wire records: int64 (n, 8) -- the bits of x y z r0 r1 r2, then id | cpu << 32, then level | grid << 32 (unsigned halves)."""
import numpy as np

REALS = ("x", "y", "z", "r0", "r1", "r2")
INTS = ("id", "cpu", "level", "grid")


def empty(n=0):
    P = {k: np.zeros(n, dtype=np.float64) for k in REALS}
    P.update({k: np.zeros(n, dtype=np.int32) for k in INTS})
    return P


def take(P, sel):
    return {k: v[sel].copy() for k, v in P.items()}


def destinations(P, level_owners, nranks, myrank):
    """(dest int32 (n), counts int32 (nranks)): the owner of the particle's box if the particle is valid and (level, grid) names a
    box of the table, else myrank"""
    n = P["id"].shape[0]
    dest = np.full(n, myrank, dtype=np.int32)
    for t in range(n):
        l, g = int(P["level"][t]), int(P["grid"][t])
        if P["id"][t] > 0 and 0 <= l < len(level_owners) and 0 <= g < len(level_owners[l]):
            dest[t] = level_owners[l][g]
    return dest, np.bincount(dest, minlength=nranks).astype(np.int32)


def _pair(lo, hi):
    return (lo.astype(np.uint32).astype(np.uint64) | (hi.astype(np.uint32).astype(np.uint64) << np.uint64(32))).view(np.int64)


def records(P):
    """the wire records of all particles of P, in order"""
    w = np.zeros((P["id"].shape[0], 8), dtype=np.int64)
    for q, k in enumerate(REALS):
        w[:, q] = P[k].view(np.int64)
    w[:, 6] = _pair(P["id"], P["cpu"])
    w[:, 7] = _pair(P["level"], P["grid"])
    return w


def pack(P, dest, nranks, myrank):
    """(kept particles, wire records): the stayers in their order; the leavers grouped by ascending destination, each group in
    its order in P"""
    kept = take(P, np.nonzero(dest == myrank)[0])
    order = np.concatenate([np.nonzero(dest == d)[0] for d in range(nranks) if d != myrank] + [np.zeros(0, dtype=np.int64)])
    return kept, records(take(P, order.astype(np.int64)))


def unpack(wire, P, at):
    """wire records into P[at, at + nrecv), in place"""
    n = wire.shape[0]
    for q, k in enumerate(REALS):
        P[k][at:at + n] = wire[:, q].view(np.float64)
    u6, u7 = wire[:, 6].view(np.uint64), wire[:, 7].view(np.uint64)
    m = np.uint64(0xffffffff)
    P["id"][at:at + n] = (u6 & m).astype(np.uint32).view(np.int32)
    P["cpu"][at:at + n] = (u6 >> np.uint64(32)).astype(np.uint32).view(np.int32)
    P["level"][at:at + n] = (u7 & m).astype(np.uint32).view(np.int32)
    P["grid"][at:at + n] = (u7 >> np.uint64(32)).astype(np.uint32).view(np.int32)


def migrate(parts, level_owners):
    """the whole migration of the particles of all ranks (parts[rank]): new parts -- on every rank the stayers in their previous
    order, then the arrivals by ascending source rank, each group in its order at the source"""
    nranks = len(parts)
    kept, wires, counts = [], [], []
    for me, P in enumerate(parts):
        dest, cnt = destinations(P, level_owners, nranks, me)
        k, w = pack(P, dest, nranks, me)
        kept.append(k)
        wires.append(w)
        counts.append(cnt)
    out = []
    for me in range(nranks):
        arrive = [(s, int(counts[s][me])) for s in range(nranks) if s != me]
        P = empty(kept[me]["id"].shape[0] + sum(c for _, c in arrive))
        nk = kept[me]["id"].shape[0]
        for k in P:
            P[k][:nk] = kept[me][k]
        at = nk
        for s, c in arrive:
            first = sum(int(counts[s][d]) for d in range(me) if d != s)
            unpack(wires[s][first:first + c], P, at)
            at += c
        out.append(P)
    return out
