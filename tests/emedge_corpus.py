"""Constructed class tables for the EM plan's hard boundaries (csrc/em.hip sfgpu_em_create, csrc/em_persist.h): record sizes, the
window's last slot and first escape, tile cuts, far-slot and fan-in limits, the overlap limit, the renumbering gate, extreme counts
and lengths, and one table that makes the plan redo itself for a crowded tile.

A case is a function -> dict(eff, rowptr, ids, counts, num_mapped, expect): the table plus the plan facts it is built to produce
(`expect`, compared key by key with EMProblem.plan_info()).  Every table keeps the builder's invariants -- labels sorted, duplicate
free, distinct, in canonical order (first id, length, bytes) -- which check_invariants() states.

plan_model() is a plain numpy restatement of the plan's RULES (the tile cut, the window, the escapes, the record sizes, the far
slots, the overlap count, the verdict) written from the comments of em.hip / em_persist.h, not a port of its kernels: tile i is the
classes whose first nonzero lies in [i T, (i+1) T); the window is [lo, lo + span) with lo the tile's smallest id and span reaching the
largest member within kWin of lo; the rest escapes.  What a case promises by hand (EXACT numbers below) is checked against the model
on the CPU (tests/test_emedge_cpu.py) and against the device (tests/test_gpu_emedges.py)."""
import numpy as np

K_WIN = 1023            # window slots 0..1022; 1023 is the null slot
K_TILE_MIN = 2048       # fewest nonzeros of a tile
K_TILE_CLS = 7800       # kTileNnz: most classes of a tile
K_TILE_MAX = 1 << 17    # kTileNnzMax
K_ESC_SLOTS = 128
K_FAN_IN = 16
K_NB_MAX = 6
K_REC = 12              # kRecSlots3
K_RENUMBER_MIN = 4096
K_SHARDS = 8
K_LDS = 81920
# persistent verdict codes: one per `return no(...)` of em_persist_check, in order
V_OK, V_NO_TABLES, V_EVENT, V_NO_HOME, V_FAN_IN, V_OVERLAP, V_LDS, V_DEVQ, V_ATTR, V_OCC, V_TILES = range(11)
V_GAVE_UP = 11          # (not the plan's: a persistent launch of the handle gave up)


def table(labels, counts, M, seed=0, eff=None):
    """labels (arrays of ids) + counts -> the case's arrays, classes put into canonical order; duplicate labels are an error"""
    labels = [np.asarray(l, np.uint32) for l in labels]
    order = sorted(range(len(labels)), key=lambda i: (int(labels[i][0]), len(labels[i]), labels[i].tobytes()))
    labels = [labels[i] for i in order]
    counts = np.asarray([counts[i] for i in order], np.uint64)
    assert len({l.tobytes() for l in labels}) == len(labels), "duplicate label"
    rp = np.zeros(len(labels) + 1, np.uint64)
    rp[1:] = np.cumsum([len(l) for l in labels])
    ids = np.concatenate(labels).astype(np.uint32) if labels else np.zeros(0, np.uint32)
    if eff is None:
        eff = np.maximum(np.random.default_rng(1000 + seed).lognormal(7.0, 0.7, M), 50.0)
    return dict(eff=np.asarray(eff, np.float64), rowptr=rp, ids=ids, counts=counts, num_mapped=int(counts.sum()), expect={})


def check_invariants(case):
    rp, ids, M = case["rowptr"].astype(np.int64), case["ids"], len(case["eff"])
    assert rp[0] == 0 and rp[-1] == len(ids) and np.all(np.diff(rp) >= 1) and len(case["counts"]) == len(rp) - 1
    assert len(ids) == 0 or int(ids.max()) < M
    prev, seen = None, set()
    for c in range(len(rp) - 1):
        l = ids[rp[c]:rp[c + 1]]
        assert np.all(np.diff(l.astype(np.int64)) > 0), f"class {c}: not sorted / duplicate member"
        key = (int(l[0]), len(l), l.tobytes())
        assert key[2] not in seen, f"class {c}: label occurs twice"
        seen.add(key[2])
        assert prev is None or prev < key, f"class {c}: out of canonical order"
        prev = key


def _counts(n, seed):
    return np.random.default_rng(seed).integers(1, 50, n).astype(np.uint64)


def plan_model(rowptr, ids, n_cu=256, gather_switch=True):
    """the plan's rules in numpy -> the facts plan_info() reports, for a table that is NOT renumbered"""
    rp = np.asarray(rowptr, np.int64); ids = np.asarray(ids, np.int64)
    C, L = len(rp) - 1, int(rp[-1])
    slots = 2 * n_cu
    tile_for = lambda r: int(min(max(-(-L // (slots * r)), K_TILE_MIN), K_TILE_MAX))
    rounds = max(1, -(-L // (slots * K_TILE_MAX)), -(-C // (slots * (K_TILE_CLS * 3 // 4))))
    T = tile_for(rounds)
    nt = max(1, -(-L // T))
    nt_small = max(1, -(-L // K_TILE_CLS)); nt_cap = max(nt, nt_small)
    redone = 0
    while True:
        c0 = np.searchsorted(rp[:C], np.arange(nt + 1, dtype=np.int64) * T, "left")
        most = int(np.max(np.diff(c0)))
        if T <= K_TILE_CLS or most <= K_TILE_CLS: break
        rounds += 1; redone += 1
        T = max(tile_for(rounds), K_TILE_CLS)
        nt = max(1, -(-L // T))
        if nt > nt_cap: nt, T = nt_small, K_TILE_CLS
    lo = np.zeros(nt, np.int64); span = np.zeros(nt, np.int64); n_esc = np.zeros(nt, np.int64); nf = np.zeros(nt, np.int64)
    n = [0, 0, 0, 0]; n_ov = 0
    feeders = {}
    for t in range(nt):
        b, e = int(rp[c0[t]]), int(rp[c0[t + 1]])
        if e == b: continue
        m = ids[b:e]
        lo[t] = m.min()
        d = m - lo[t]
        far = d >= K_WIN
        span[t] = d[~far].max() + 1
        n_esc[t] = far.sum()
        tg = np.unique(m[far]); nf[t] = len(tg)
        for x in tg: feeders[int(x)] = feeders.get(int(x), 0) + 1
        cls = np.repeat(np.arange(c0[t + 1] - c0[t]), np.diff(rp[c0[t]:c0[t + 1] + 1]))
        nc = int(c0[t + 1] - c0[t])
        n_in = np.bincount(cls[~far], minlength=nc); has_far = np.bincount(cls[far], minlength=nc) > 0
        b4 = has_far | (n_in > K_REC)
        n[0] += int(np.sum(~b4 & (n_in <= 3))); n[1] += int(np.sum(~b4 & (n_in > 3) & (n_in <= 6)))
        n[2] += int(np.sum(~b4 & (n_in > 6))); n[3] += int(b4.sum())
        n_ov += int(np.sum((n_in[n_in > K_REC] - 1) // K_REC))
    P, E = int(span.sum()), int(n_esc.sum())
    live = span > 0
    cover = 0
    for t in np.nonzero(live)[0]:
        ov = live & (lo + span > lo[t]) & (lo < lo[t] + span[t])
        if int(ov.sum()) - 1 > K_NB_MAX: cover += 1
    lo_live = lo[live]
    monotone = bool(np.all(np.diff(lo_live) >= 0))
    gather = bool(gather_switch and L > E)
    homes = np.zeros(int(ids.max()) + 2 if L else 1, bool)
    for t in np.nonzero(live)[0]: homes[lo[t]:lo[t] + span[t]] = True
    info = dict(n_tiles=nt, tile_nnz=T, redone=redone, most_classes=most, P=P, E=E, renumbered=0, gather=int(gather),
                cover_tiles=cover if gather else 0, fused_ok=int(gather and monotone))
    tables = gather and nt <= 4096 and 2 * P * 16 + 3 * E * 16 < (1 << 31)
    if tables:
        far_cap = int(nf.max()); info.update(most_far_slots=far_cap, longest_far_list=int(n_esc.max()) if E else 0,
                                             n1=n[0], n2=n[1], n3=n[2], n4=n[3], n_ov=n_ov)
        base = (2 * (K_WIN + 2) + (most + 2) + 2 * far_cap + 2 * 16) * 8 + 32 + 4 * K_SHARDS * 4 + ((most + 2) + far_cap + (K_WIN if E else 0) + 1) * 4
        if any(not homes[x] for x in feeders): v = V_NO_HOME
        elif any(k > K_FAN_IN for k in feeders.values()): v = V_FAN_IN
        elif cover: v = V_OVERLAP
        elif base + 64 > K_LDS: v = V_LDS
        elif nt > 2 * n_cu: v = V_TILES
        else: v = V_OK
    else:
        info.update(most_far_slots=0, longest_far_list=0, n1=0, n2=0, n3=0, n4=0, n_ov=0)
        v = V_NO_TABLES
    info["persist_verdict"] = v
    info["_tile"] = dict(c0=c0, lo=lo, span=span, n_esc=n_esc, nf=nf)
    return info


def _local4(first_ids):
    """classes of 4 neighbouring transcripts, one per first id: [f, f+1, f+3, f+6] (distinct for distinct f)"""
    return [np.array([f, f + 1, f + 3, f + 6]) for f in first_ids]


def _fill(base, nnz):
    """classes with first ids base, base + 1, ... that hold exactly `nnz` nonzeros: classes of 4 and one of 2 or 3 (or 5) for the rest"""
    assert nnz >= 2
    n4, r = divmod(nnz, 4)
    if r == 1: n4 -= 1; r = 5
    out = _local4(base + np.arange(n4))
    f = base + n4
    if r == 2: out.append(np.array([f, f + 2]))
    elif r == 3: out.append(np.array([f, f + 2, f + 4]))
    elif r == 5: out.append(np.array([f, f + 1, f + 2, f + 4, f + 7]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
def tiny(M, C):
    """(1,1) all singletons; (2,1); (3,2) with transcript 1 in no class; (64,3) / (65,3): a class of every transcript"""
    labels = {(1, 1): [[0]], (2, 1): [[0, 1]], (3, 2): [[0], [0, 2]],
              (64, 3): [np.arange(64), [0, 1], [63]], (65, 3): [np.arange(65), [5], [64]]}[(M, C)]
    case = table(labels, _counts(C, M), M, seed=M)
    n_in = [len(l) for l in labels]
    case["expect"] = dict(n_tiles=1, tile_nnz=2048, redone=0, most_classes=C, E=0, P=max(int(np.max(l)) for l in labels) - min(int(np.min(l)) for l in labels) + 1,
                          renumbered=0, gather=1, cover_tiles=0, most_far_slots=0, fused_ok=1, persist_verdict=V_OK,
                          n1=sum(k <= 3 for k in n_in), n2=0, n3=0, n4=sum(k > 12 for k in n_in), n_ov=sum((k - 1) // 12 for k in n_in if k > 12))
    return case


REC_SIZES = (1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 24, 25, 36, 37, 100)


def record_sizes(odd):
    """one tile, three classes of every size of REC_SIZES, all members inside the window; `odd` adds one more singleton, so the tile's
    class count -- den_cap, on whose parity the persistent kernel's LDS carve depends -- is 48 or 49"""
    rng = np.random.default_rng(41)
    sizes = [k for k in REC_SIZES for _ in range(3)] + ([1] if odd else [])
    rng.shuffle(sizes)
    labels = []
    for j, k in enumerate(sizes):                      # first id j: distinct labels, canonical order = this order
        rest = np.sort(rng.choice(np.arange(j + 1, 1000), k - 1, replace=False)) if k > 1 else np.zeros(0, int)
        labels.append(np.concatenate([[j], rest]))
    case = table(labels, _counts(len(labels), 42), 1010, seed=2)
    k = np.asarray(sizes)
    case["expect"] = dict(n_tiles=1, tile_nnz=2048, redone=0, most_classes=len(sizes), E=0, renumbered=0, gather=1, cover_tiles=0,
                          most_far_slots=0, longest_far_list=0, fused_ok=1, persist_verdict=V_OK,
                          n1=int(np.sum(k <= 3)), n2=int(np.sum((k > 3) & (k <= 6))), n3=int(np.sum((k > 6) & (k <= 12))),
                          n4=int(np.sum(k > 12)), n_ov=int(np.sum((k[k > 12] - 1) // 12)))
    assert case["expect"]["n4"] == 21 and case["expect"]["n_ov"] == 54 and case["expect"]["most_classes"] == 48 + int(odd)
    return case


def window_edge():
    """classes whose last member sits at window base + 1021, + 1022 (the last slot), + 1023 (the null slot's number: the first escape)
    and + 1024, a pair and a class of five for each, in tile 0 (base 0) and in tile 1 (base 1023).  Tile 0 holds exactly 2048 nonzeros
    of first ids below 1023, starting at the singleton [0], and tile 1 starts at the singleton [1023], so the bases are exact; tile 2 starts at [2046] and gives the
    second tile's far members their home.  E = 2 tiles x 2 offsets x 2 classes."""
    labels = []
    for base, nxt in ((0, 1023), (1023, 2046)):
        edge = []
        for j, k in enumerate((1021, 1022, 1023, 1024)):
            a = base + 3 + 20 * j
            edge.append(np.array([a, base + k])); edge.append(np.array([a + 1, a + 2, a + 4, a + 9, base + k]))
        homes = [np.array([base]), np.array([base + 1])]      # (they pin the tile's base; tile 1's are the homes of tile 0's far members 1023, 1024)
        used = sum(len(l) for l in edge) + len(homes)
        labels += homes + edge + _fill(base + 100, 2048 - used)
    labels += [np.array([2046]), np.array([2047]), np.array([2046, 2050]), np.array([2047, 2049, 2051])]
    case = table(labels, _counts(len(labels), 43), 2100, seed=3)
    case["expect"] = dict(n_tiles=3, tile_nnz=2048, redone=0, E=8, P=1023 + 1023 + 6, renumbered=0, gather=1, cover_tiles=0, most_far_slots=2,
                          longest_far_list=4, fused_ok=1, persist_verdict=V_OK)
    return case


def tile_cut(k, d):
    """rp_end = 2048 k + d from classes of 4 (and one of 3 / 5 for the odd totals).  d = +1: the last nominal tile holds the last
    nonzero of a class that started before the cut, so it has no class of its own (an empty tile)"""
    labels = _fill(0, 2048 * k + d)
    case = table(labels, _counts(len(labels), 44 + k), len(labels) + 10, seed=4)
    case["expect"] = dict(n_tiles=k + (d > 0), tile_nnz=2048, redone=0, E=0, renumbered=0, gather=1, cover_tiles=0, fused_ok=1, persist_verdict=V_OK,
                          most_classes=512, n1=int(d == -1), n2=512 * k - int(d == -1), n3=0, n4=0, n_ov=0)      # (the class of 3 is a 4-byte record, the class of 5 an 8-byte one)
    return case


def tile_straddle():
    """a class that lies across the nominal cut at 2048 (nonzeros 2046 .. 2049): it belongs to tile 0, tile 1 starts behind it"""
    labels = _fill(0, 2046) + [np.array([600, 601, 603, 605])] + _fill(700, 1000)
    case = table(labels, _counts(len(labels), 48), 1000, seed=5)
    case["expect"] = dict(n_tiles=2, tile_nnz=2048, redone=0, E=0, renumbered=0, gather=1, cover_tiles=0, fused_ok=1, persist_verdict=V_OK,
                          most_classes=513)
    return case


def tile_long():
    """one class of 2049 members and one of 5000 among classes of 5 (about 410 to a tile, on every second id: windows of some 830
    transcripts that leave no transcript without a home): longer than the smallest tile and longer than the window, so both
    escape (2049 - 1023 and 5000 - 1023 far members at least), tiles behind them are empty, and the far slots of the 5000-class's tile
    do not fit the persistent loop's LDS: the verdict is the LDS code and the run takes the fused iteration"""
    labels = [np.array([f, f + 1, f + 2, f + 4, f + 7]) for f in 2 * np.arange(3005)] + [np.arange(0, 2049), np.arange(1000, 6000)]
    case = table(labels, _counts(len(labels), 49), 6020, seed=6)
    case["expect"] = dict(tile_nnz=2048, redone=0, renumbered=0, gather=1, fused_ok=1, persist_verdict=V_LDS)
    return case


def esc_slots(n):
    """tile 0 (exactly 2048 nonzeros, base 0) has n distinct far transcripts 2000 .. 2000 + n - 1, one pair class each; tile 1 starts at
    the singleton [2000] and holds a singleton of every target.  kEscSlots = 128: the 129th goes straight to alphaOut"""
    far = [np.array([2 * j, 2000 + j]) for j in range(n)]
    labels = far + _fill(300, 2048 - 2 * n) + [np.array([2000 + j]) for j in range(n)] + _fill(2000, 40)
    case = table(labels, _counts(len(labels), 50 + n), 2200, seed=7)
    case["expect"] = dict(n_tiles=2, tile_nnz=2048, redone=0, E=n, renumbered=0, gather=1, cover_tiles=0, most_far_slots=n, longest_far_list=n,
                          fused_ok=1, persist_verdict=V_OK)
    return case


def fan_in(n):
    """n full tiles (bases 0, 600, ...), each with one pair class whose second member is transcript X far beyond every window; X's
    home is the last tile (a singleton [X] and a neighbour).  kFanInMax = 16"""
    X = 600 * n + 2000
    labels = []
    for t in range(n):
        labels += [np.array([600 * t, X])] + _fill(600 * t, 2046)
    labels += [np.array([X]), np.array([X, X + 1, X + 2])]
    case = table(labels, _counts(len(labels), 60 + n), X + 10, seed=8)
    case["expect"] = dict(n_tiles=n + 1, tile_nnz=2048, redone=0, E=n, renumbered=0, gather=1, cover_tiles=0, most_far_slots=1, longest_far_list=1,
                          fused_ok=1, persist_verdict=V_OK if n <= K_FAN_IN else V_FAN_IN)
    return case


def far_home(with_home):
    """tile 0 (2048 nonzeros, base 0) has a far member 3000; tile 1 (base 2000) reaches 2010 without and 3000 with the singleton [3000]"""
    labels = [np.array([5, 3000])] + _fill(0, 2046) + _fill(2000, 8) + ([np.array([3000])] if with_home else [])
    case = table(labels, _counts(len(labels), 70), 3010, seed=9)
    case["expect"] = dict(n_tiles=2, tile_nnz=2048, redone=0, E=1, renumbered=0, gather=1, cover_tiles=0, most_far_slots=1, fused_ok=1,
                          persist_verdict=V_OK if with_home else V_NO_HOME)
    return case


def overlap(n):
    """n tiles of 2048 nonzeros (512 classes of 4) whose windows all lie in one band of 900 transcripts and all overlap each other:
    every tile is overlapped by n - 1.  kNbMax = 6"""
    rng = np.random.default_rng(90 + n)
    nC = 512 * n
    labels, seen = [], set()
    for q in range(nC):
        f = q * 860 // nC
        while True:
            l = np.concatenate([[f], np.sort(rng.choice(np.arange(f + 1, 899), 3, replace=False))])
            if q % 64 == 0: l[3] = 899                    # every tile's window reaches the band's end
            if l.tobytes() not in seen: break
        seen.add(l.tobytes()); labels.append(l)
    case = table(labels, _counts(nC, 91), 900, seed=10)
    case["expect"] = dict(n_tiles=n, tile_nnz=2048, redone=0, E=0, renumbered=0, gather=1, fused_ok=1, most_classes=512,
                          persist_verdict=V_OK if n - 1 <= K_NB_MAX else V_OVERLAP)
    case["expect"]["cover_tiles"] = 0 if n - 1 <= K_NB_MAX else n
    return case


def renumber_gate(C):
    """512 groups of 8 transcripts, each with 8 classes of its own (a chain of 7 pairs and one triple that closes it: any two members
    are at most 4 class hops apart), under a random permutation of the ids: in the caller's order most members lie outside their
    tile's window, in the plan's own order (transcripts by the smallest id within 5 hops) every group is contiguous.  C = 4096 is
    kRenumberMinClasses; 4095 is the same table without its last class"""
    rng = np.random.default_rng(77)
    G = 512
    perm = rng.permutation(8 * G)
    labels = []
    for g in range(G):
        t = perm[8 * g:8 * g + 8]
        labels += [np.sort([t[i], t[i + 1]]) for i in range(7)] + [np.sort([t[0], t[3], t[7]])]
    case = table(labels, _counts(len(labels), 78), 8 * G, seed=11)
    if C < len(labels):
        keep = C
        case = dict(case, rowptr=case["rowptr"][:keep + 1], ids=case["ids"][:int(case["rowptr"][keep])], counts=case["counts"][:keep])
        case["num_mapped"] = int(case["counts"].sum())
    case["expect"] = dict(renumbered=int(C >= K_RENUMBER_MIN), gather=1, redone=0, tile_nnz=2048, n_tiles=5)
    if C >= K_RENUMBER_MIN:          # (in the plan's own order a group's 8 transcripts are neighbours: nothing escapes, and the plan is eligible)
        case["expect"].update(E=0, fused_ok=1, cover_tiles=0, most_far_slots=0, persist_verdict=V_OK)
    return case


def extremes():
    """counts 1 and 2^31 - 1, effective lengths 0.5 (clamped to 1) and 1e9, zero-count SINGLETON classes between live ones ([3], [20]:
    well defined under EM and VBEM alike), and transcripts whose alpha ends at or below the truncation cut-off: 12 and 23 (1e9 long,
    next to short ones: towards 0 under EM, towards the prior under VBEM within a few iterations) and 20 (its only class has count 0)"""
    labels = [[0], [0, 1], [1, 2, 3], [2, 30], [3], [3, 4], [4, 5, 6, 7], [5], [6, 9], [8, 9], [9, 10, 11], [10], [12, 13], [13, 14, 15],
              [20], [22, 23], [23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37]]
    counts = [1, (1 << 31) - 1, 7, 2, 0, 1, 1000, (1 << 31) - 1, 11, 3, 1, 1, 5, 4, 0, 2, 9]
    M = 40
    eff = np.maximum(np.random.default_rng(5).lognormal(7.0, 0.7, M), 50.0)
    eff[1] = 0.5; eff[4] = 1e9; eff[9] = 0.5; eff[12] = 1e9; eff[23] = 1e9
    case = table([np.array(l) for l in labels], counts, M, eff=eff)
    case["expect"] = dict(n_tiles=1, tile_nnz=2048, redone=0, E=0, renumbered=0, gather=1, cover_tiles=0, fused_ok=1, persist_verdict=V_OK,
                          most_classes=len(labels))
    case["truncated"] = [12, 20, 23]
    return case


def extremes_zero_counts():
    """zero-count classes of two and three members (and singletons) between live ones; transcripts 20 and 21 are members of
    zero-count classes only: active, alpha = 0 (EM) or the prior (VBEM) after one iteration, truncated at the end.  The stored weights
    of such a class are 0 / 0: EMUpdate_ skips them ("if (!std::isnan(v))", :269), VBEMUpdate_ (:340-361) does not, so under VBEM the
    reference -- and the C oracle, which follows it -- returns NaN.  The kernels never form the stored weights: a zero-count class
    contributes nothing in either mode (the contract of include/sfgpu.h).  Under VBEM this case is therefore held to mpmath with
    skip_zero_count and, for the stop iteration, to the numpy restatement, which skips such a class as well"""
    labels = [[0], [0, 1], [1, 2, 3], [2, 30], [3, 4], [4, 5, 6, 7], [5], [6, 9], [8, 9], [9, 10, 11], [10], [12, 13], [13, 14, 15],
              [20, 21], [20], [22, 23], [23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37]]
    counts = [1, 40, 7, 0, 1, 1000, 17, 0, 3, 1, 1, 5, 0, 0, 0, 2, 9]
    case = table([np.array(l) for l in labels], counts, 40, seed=12)
    case["expect"] = dict(n_tiles=1, tile_nnz=2048, redone=0, E=0, renumbered=0, gather=1, cover_tiles=0, fused_ok=1, persist_verdict=V_OK,
                          most_classes=len(labels))
    case["truncated"] = [20, 21]
    case["vbem_zero_count"] = True           # (VBEM: the oracle is NaN here, see above)
    return case


def crowded_tile(n_cu):
    """the one large table: a run of singletons longer than a nominal tile, then classes of 15, rp_end just above 2 CUs 7800 nonzeros:
    the nominal tile (rp_end / (2 CUs), a little over 7800) then holds more than 7800 classes and the plan is redone with one more round.
    (A tile of 7800 singletons spans 7800 transcripts: all but the window's 1023 are far members without a home, so the plan is not
    eligible for the persistent loop either -- plan_model says which verdict)"""
    slots = 2 * n_cu
    S = 12000
    n15 = (slots * K_TILE_CLS + 200 - S) // 15 + 1
    M = S + n15 + 40
    first = S + np.arange(n15, dtype=np.int64)
    off = np.array([0, 1, 2, 3, 4, 6, 7, 9, 11, 12, 15, 17, 20, 24, 29], np.int64)
    ids = np.concatenate([np.arange(S, dtype=np.int64), (first[:, None] + off[None, :]).ravel()]).astype(np.uint32)
    rp = np.concatenate([np.arange(S, dtype=np.uint64), S + 15 * np.arange(n15 + 1, dtype=np.uint64)])
    counts = _counts(S + n15, 99)
    eff = np.maximum(np.random.default_rng(98).lognormal(7.0, 0.7, M), 50.0)
    case = dict(eff=eff, rowptr=rp, ids=ids, counts=counts, num_mapped=int(counts.sum()), expect={})
    case["expect"] = dict(redone=1, tile_nnz=K_TILE_CLS, renumbered=0, gather=1)
    return case


# every case but crowded_tile (which needs the device's CU count): name -> constructor
CASES = {}
for _mc in ((1, 1), (2, 1), (3, 2), (64, 3), (65, 3)): CASES[f"tiny_{_mc[0]}_{_mc[1]}"] = (lambda mc=_mc: tiny(*mc))
CASES["record_sizes_even"] = lambda: record_sizes(False)
CASES["record_sizes_odd"] = lambda: record_sizes(True)
CASES["window_edge"] = window_edge
for _k in (1, 2, 3):
    for _d in (-1, 0, 1): CASES[f"tile_cut_{_k}_{'m1' if _d < 0 else 'p1' if _d > 0 else '0'}"] = (lambda k=_k, d=_d: tile_cut(k, d))
CASES["tile_straddle"] = tile_straddle
CASES["tile_long"] = tile_long
for _n in (127, 128, 129): CASES[f"esc_slots_{_n}"] = (lambda n=_n: esc_slots(n))
for _n in (16, 17): CASES[f"fan_in_{_n}"] = (lambda n=_n: fan_in(n))
CASES["far_home_none"] = lambda: far_home(False)
CASES["far_home_singleton"] = lambda: far_home(True)
for _n in (7, 8): CASES[f"overlap_{_n}"] = (lambda n=_n: overlap(n))
for _c in (4095, 4096): CASES[f"renumber_gate_{_c}"] = (lambda c=_c: renumber_gate(c))
CASES["extremes"] = extremes
CASES["extremes_zero_counts"] = extremes_zero_counts


# ------------------------------------------------------------------------------------------------------------------------------
# The reference side, shared by the CPU and the GPU tests: mpmath (50 digits) after 1, 2 and 5 iterations and -- where the table
# is small enough -- at the oracle's stop iteration; the C oracle on the same table; and the oracle's own distance to mpmath,
# the yardstick of the device's bound.
FIXED_ITERS = (1, 2, 5)
FLOOR = 64 * 2.0 ** -53
SUITE_BOUND = 1e-9
CUTOFF = {False: 1e-8, True: 0.01 + 1e-8}


def truncate(alpha, vb):
    return np.where(alpha <= CUTOFF[vb], 0.0, alpha)


def mass_of(alpha):
    s = float(np.sum(alpha.astype(np.longdouble)))
    return alpha / s if s > 0 else alpha


def rel_dist(a, ref):
    """largest relative distance over the reference's support; the supports must be equal"""
    nz = ref > 0
    assert np.array_equal(a > 0, nz), "support differs"
    return float(np.max(np.abs(a[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0


def clear_of_cutoff(alpha_mp, vb):
    """no untruncated mpmath value within 1e-14 of the truncation cut-off (1e-8 above 0, or above the prior under VBEM, where a
    transcript without reads sits at the prior exactly): 1e-6 of the cut-off's own 1e-8, a thousand times the suite's 1e-9 -- the
    support is then the same in every arithmetic the suite accepts"""
    return bool(np.all(np.abs(alpha_mp - CUTOFF[vb]) > 1e-14))


def bound_for(dist):
    """the device's bound against mpmath: 8 x the oracle's own distance, at least 64 ulp, never more than the suite's 1e-9"""
    return min(max(8.0 * dist, FLOOR), SUITE_BOUND)


def serial_run(case, vb, tol=0.01, min_iter=50, max_iter=10000):
    """the serial side of the reference: the C oracle -> (alpha, mass, stats); for VBEM on a table with zero-count classes of several
    members, where the oracle follows the reference into NaN, the numpy restatement (which skips such a class) in the oracle's place"""
    eff, rp, ii, cc, N = case["eff"], case["rowptr"], case["ids"], case["counts"], case["num_mapped"]
    if not (vb and case.get("vbem_zero_count")):
        from oracle import oracle as O
        rc, oa, om, st = O.em_optimize(eff, rp, ii, cc, N, use_vbem=vb, tol=tol, min_iter=min_iter, max_iter=max_iter)
        assert rc == 0
        return oa, om, st
    import em_numpy_restatement as R
    with np.errstate(all="ignore"):
        p = R.Problem(eff, rp, ii, cc, N)
        alpha, it, conv, mrd = p.alpha0(), 0, False, 0.0
        while it < min_iter or (it < max_iter and not conv):
            new = p.step(alpha, True)
            gate = new > R.ALPHA_CHECK_CUTOFF
            rel = np.abs(alpha[gate] - new[gate]) / new[gate]
            mrd = float(rel.max()) if rel.size else 0.0
            conv = mrd <= tol
            alpha = new; it += 1
    t = truncate(alpha, True)
    return t, mass_of(t), dict(iters=it, converged=bool(conv), max_rel_diff=mrd, alpha_sum=float(t.sum()), n_active=p.n_active)


_REF = {}


def reference(name, case=None):
    """-> {vb: {"fixed": {n: dict(mp_raw, mp, mp_mass, oracle, oracle_mass, stats, dist)}, "conv": the same + prev_stats}}: mpmath after
    1, 2, 5 iterations (computed) and at the serial side's stop iteration (RECORDED, see below), the serial side on the same table,
    and its distance to mpmath -- the yardstick of the device's bound.  Once per process and table."""
    if name in _REF: return _REF[name]
    import em_numpy_restatement as R
    case = case or CASES[name]()
    eff, rp, ii, cc, N = case["eff"], case["rowptr"], case["ids"], case["counts"], case["num_mapped"]
    gold = np.load(golden_path(name))
    assert str(gold["digest"]) == table_digest(case), f"{name}: the table no longer matches tests/golden/emedge/{name}.npz -- run python tests/emedge_corpus.py {name}"
    out = {}
    for vb in (False, True):
        mp = R.optimize_mp(eff, rp.astype(np.int64), ii, cc, N, vb=vb, keep=FIXED_ITERS, skip_zero_count=bool(case.get("vbem_zero_count")))
        fixed = {}
        for n in FIXED_ITERS:
            oa, om, st = serial_run(case, vb, tol=0.0, min_iter=n, max_iter=n)
            t = truncate(mp[n], vb); tm = mass_of(t)
            fixed[n] = dict(mp_raw=mp[n], mp=t, mp_mass=tm, oracle=oa, oracle_mass=om, stats=st, dist=max(rel_dist(oa, t), rel_dist(om, tm)))
        oa, om, st = serial_run(case, vb)
        it = st["iters"]
        _, _, prev = serial_run(case, vb, min_iter=min(50, it - 1), max_iter=it - 1)
        tag = "vb_" if vb else "em_"
        assert int(gold[tag + "iters"]) == it, f"{name}: recorded at iteration {int(gold[tag + 'iters'])}, the serial side stops at {it}"
        raw = gold[tag]
        t = truncate(raw, vb); tm = mass_of(t)
        out[vb] = dict(fixed=fixed, conv=dict(mp_raw=raw, mp=t, mp_mass=tm, oracle=oa, oracle_mass=om, stats=st, prev_stats=prev,
                                               dist=max(rel_dist(oa, t), rel_dist(om, tm))))
    _REF[name] = out
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# The converged runs' mpmath results are RECORDED (tests/golden/emedge/<case>.npz): restating several hundred iterations of a
# 30 000-nonzero table in 50-digit arithmetic takes minutes, which no test run should pay.  A record holds optimize_mp's alpha at the
# oracle's stop iteration for EM and VBEM, those iterations, and a digest of the table it was made from -- a table that no longer
# matches its record fails the tests until `python tests/emedge_corpus.py` has been run again (about ten minutes on eight cores).
def table_digest(case):
    import hashlib
    h = hashlib.sha256()
    for k in ("eff", "rowptr", "ids", "counts"): h.update(np.ascontiguousarray(case[k]).tobytes())
    h.update(str(case["num_mapped"]).encode())
    return h.hexdigest()


def golden_path(name):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emedge", name + ".npz")


def _record_job(job):
    import sys, os
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path: sys.path.insert(0, p)
    import em_numpy_restatement as R
    name, vb, it = job
    case = CASES[name]()
    raw = R.optimize_mp(case["eff"], case["rowptr"].astype(np.int64), case["ids"], case["counts"], case["num_mapped"], vb=vb, n_iter=it,
                        skip_zero_count=bool(case.get("vbem_zero_count")))
    return name, vb, it, raw


def record_golden(names=None, procs=8):
    import multiprocessing as mpr, os, sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path: sys.path.insert(0, p)
    jobs = []
    for name in (names or sorted(CASES)):
        case = CASES[name]()
        for vb in (False, True):
            _, _, st = serial_run(case, vb)
            jobs.append((name, vb, st["iters"], int(case["rowptr"][-1]) + len(case["eff"])))
    jobs.sort(key=lambda j: -j[2] * j[3])
    out = {}
    with mpr.Pool(procs) as pool:
        for name, vb, it, raw in pool.imap_unordered(_record_job, [j[:3] for j in jobs]):
            out.setdefault(name, {})[vb] = (it, raw)
            case = CASES[name]()
            if len(out[name]) == 2:
                os.makedirs(os.path.dirname(golden_path(name)), exist_ok=True)
                rec = dict(digest=np.array(table_digest(case)))
                for v, (i, r) in out[name].items(): rec["vb_" if v else "em_"] = r; rec["vb_iters" if v else "em_iters"] = np.array(i)
                np.savez_compressed(golden_path(name), **rec)
                print("recorded", name, {("VBEM" if v else "EM"): i for v, (i, r) in out[name].items()}, flush=True)


if __name__ == "__main__":
    import sys
    record_golden(sys.argv[1:] or None)
