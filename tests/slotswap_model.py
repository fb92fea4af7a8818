"""numpy model of the timeslot-swap descent (include/ttga_slotswap.h).

Two forms of delta(a, b), the change of scv when the events of slots a and b
trade places:
  deltas_brute  exchanges the two slots in the row and recomputes scv from
                the definitions (scv_of, itself checked against ttga.validate);
  deltas_table  the kernel's formulation: att^T . D over the students for the
                pairs on different days, the day's 9 bits exchanged for the
                pairs on one day, the last-slot term from the slots' weights;
  deltas_windows  deltas_table with the pairs on one day from co-occurrence
                counts of the windows of three, as the kernel contracts them.
  deltas_lut    the same deltas from a 512-entry table of h over the nine bits
                of a day: D by table lookup and att^T . D as one float64
                product (exact: its sums stay far below 2^53), the pairs on
                one day from the count of each day pattern. Shares no step
                with the kernel's contractions and takes milliseconds where
                the other forms take seconds (S in the tens of thousands).
descend() is the steepest descent with the header's tie rule."""
import numpy as np

SLOTS, PER_DAY, DAYS = 45, 9, 5
PAIRS = [(a, b) for a in range(SLOTS) for b in range(a + 1, SLOTS)]
NO_PAIR = np.iinfo(np.int64).max


def load_golden(name):
    """The instance of tests/golden/<name>.npz."""
    import pathlib

    import ttga
    z = np.load(pathlib.Path(__file__).resolve().parent / "golden" / f"{name}.npz")
    E, R, F, S = (int(x) for x in z["dims"])
    return ttga.Instance(E, R, F, S, z["room_size"], z["student_events"], z["room_features"], z["event_features"])


def attendance(inst, slot):
    """att[s][t] = student s has a class in slot t (bool [S, 45])."""
    X = np.zeros((inst.E, SLOTS), np.float32)
    X[np.arange(inst.E), np.asarray(slot, np.int64)] = 1
    return (inst.student_events.astype(np.float32) @ X) > 0


def weights(inst, slot):
    """W[t] = the sum of studentNumber over the events in slot t."""
    sn = inst.student_events.astype(np.int64).sum(axis=0)
    return np.bincount(np.asarray(slot, np.int64), weights=sn, minlength=SLOTS).astype(np.int64)


def day_cost(days):
    """h per (student, day): windows of three classes in a row + [exactly one class]; days bool [..., 9]."""
    return ((days[..., :-2] & days[..., 1:-1] & days[..., 2:]).sum(axis=-1) + (days.sum(axis=-1) == 1)).astype(np.int64)


def scv_of(inst, slot):
    slot = np.asarray(slot, np.int64)
    last = int(weights(inst, slot)[PER_DAY - 1::PER_DAY].sum())
    return last + int(day_cost(attendance(inst, slot).reshape(inst.S, DAYS, PER_DAY)).sum())


def swapped(slot, a, b):
    slot = np.asarray(slot)
    out = slot.copy()
    out[slot == a] = b
    out[slot == b] = a
    return out


def deltas_brute(inst, slot):
    """int64 [45, 45]; entries a < b hold delta(a, b), the rest NO_PAIR."""
    d = np.full((SLOTS, SLOTS), NO_PAIR, np.int64)
    base = scv_of(inst, slot)
    for a, b in PAIRS:
        d[a, b] = scv_of(inst, swapped(slot, a, b)) - base
    return d


def d_table(att):
    """D[s][9d + k] = h(m_d | bit k) - h(m_d & ~bit k), int64 [S, 45]."""
    days = att.reshape(-1, DAYS, PER_DAY)
    D = np.zeros(days.shape, np.int64)
    for k in range(PER_DAY):
        on, off = days.copy(), days.copy()
        on[:, :, k] = True
        off[:, :, k] = False
        D[:, :, k] = day_cost(on) - day_cost(off)
    return D.reshape(-1, SLOTS)


def deltas_table(inst, slot):
    att = attendance(inst, slot)
    W = weights(inst, slot)
    D = d_table(att)
    assert D.min(initial=0) >= -1 and D.max(initial=0) <= 3           # fits the int8 operand
    T = att.astype(np.int64).T @ D                                    # T[b][a] = sum_s att[s][b] D[s][a]
    days = att.reshape(-1, DAYS, PER_DAY)
    base = day_cost(days)
    last = (np.arange(SLOTS) % PER_DAY == PER_DAY - 1).astype(np.int64)
    diag = np.diagonal(T)
    v = T + T.T - diag[:, None] - diag[None, :]                       # v[a][b], valid across days
    for ka in range(PER_DAY):                                         # one day: both bits exchanged
        for kb in range(ka + 1, PER_DAY):
            sw = days.copy()
            sw[:, :, [ka, kb]] = sw[:, :, [kb, ka]]
            same = (day_cost(sw) - base).sum(axis=0)                  # [5], per day
            v[PER_DAY * np.arange(DAYS) + ka, PER_DAY * np.arange(DAYS) + kb] = same
    v = v + (W[None, :] - W[:, None]) * (last[:, None] - last[None, :])
    return np.where(np.triu(np.ones((SLOTS, SLOTS), bool), k=1), v, NO_PAIR)


def pair_columns(att):
    """The kernel's second operand for the pairs on one day, int64 [S, 5, 15]:
    columns 0..7 of a day = the student attends positions i and i + 1, columns
    8..14 = positions i and i + 2."""
    days = att.reshape(-1, DAYS, PER_DAY)
    return np.concatenate([days[:, :, :-1] & days[:, :, 1:], days[:, :, :-2] & days[:, :, 2:]], axis=2).astype(np.int64)


def same_day_windows(att):
    """delta of the pairs on one day from co-occurrence counts, the form the
    kernel contracts by MFMA: N3[d][t][c] = the students in position t of day d
    and in both positions of pair column c. Exchanging two bits of a day keeps
    its number of classes, so only the windows of three change, and of those
    only the ones that hold exactly one of the two positions: there the
    position's bit is replaced by the other's. Returns {(a, b): delta} without
    the last-slot term."""
    days = att.reshape(-1, DAYS, PER_DAY).astype(np.int64)
    N3 = np.einsum("sdt,sdc->dtc", days, pair_columns(att))

    def moved(d, k, other):
        """The windows that hold k and not `other`, with k's bit replaced by other's."""
        v = 0
        for w in (k - 2, k - 1, k):
            if 0 <= w <= PER_DAY - 3 and not w <= other <= w + 2:
                c = k + 1 if w == k else 8 + k - 1 if w == k - 1 else k - 2
                v += N3[d, other, c] - N3[d, k, c]
        return v
    return {(PER_DAY * d + ka, PER_DAY * d + kb): int(moved(d, ka, kb) + moved(d, kb, ka))
            for d in range(DAYS) for ka in range(PER_DAY) for kb in range(ka + 1, PER_DAY)}


def deltas_windows(inst, slot):
    """deltas_table with the pairs on one day from same_day_windows: both
    contractions of the kernel and nothing else (the quickest of the three)."""
    att = attendance(inst, slot)
    W = weights(inst, slot)
    T = att.astype(np.int64).T @ d_table(att)
    diag = np.diagonal(T)
    v = T + T.T - diag[:, None] - diag[None, :]
    for (a, b), same in same_day_windows(att).items():
        v[a, b] = same
    last = (np.arange(SLOTS) % PER_DAY == PER_DAY - 1).astype(np.int64)
    v = v + (W[None, :] - W[:, None]) * (last[:, None] - last[None, :])
    return np.where(np.triu(np.ones((SLOTS, SLOTS), bool), k=1), v, NO_PAIR)


def _day_tables():
    """H[i] = h of the day whose bit k is position k of i; DL[i][k] = H[i | bit k]
    - H[i & ~bit k]; SW[i][c] = H[i with the bits of pair c exchanged] - H[i]."""
    i = np.arange(1 << PER_DAY)
    H = day_cost(((i[:, None] >> np.arange(PER_DAY)) & 1).astype(bool))
    DL = np.stack([H[i | (1 << k)] - H[i & ~(1 << k)] for k in range(PER_DAY)], axis=1)
    pairs = [(ka, kb) for ka in range(PER_DAY) for kb in range(ka + 1, PER_DAY)]
    SW = np.stack([H[np.where(((i >> ka) ^ (i >> kb)) & 1, i ^ ((1 << ka) | (1 << kb)), i)] - H for ka, kb in pairs],
                  axis=1)
    return DL, SW, pairs


_DAY_TABLES = _day_tables()


def deltas_lut(inst, slot):
    DL, SW, pairs = _DAY_TABLES
    att = attendance(inst, slot)
    W = weights(inst, slot)
    idx = att.reshape(-1, DAYS, PER_DAY).astype(np.int64) @ (1 << np.arange(PER_DAY))       # [S, 5]
    D = DL[idx].reshape(-1, SLOTS)
    T = np.rint(att.astype(np.float64).T @ D.astype(np.float64)).astype(np.int64)
    diag = np.diagonal(T)
    v = T + T.T - diag[:, None] - diag[None, :]
    for d in range(DAYS):
        same = np.bincount(idx[:, d], minlength=1 << PER_DAY).astype(np.int64) @ SW
        for (ka, kb), dl in zip(pairs, same):
            v[PER_DAY * d + ka, PER_DAY * d + kb] = dl
    last = (np.arange(SLOTS) % PER_DAY == PER_DAY - 1).astype(np.int64)
    v = v + (W[None, :] - W[:, None]) * (last[:, None] - last[None, :])
    return np.where(np.triu(np.ones((SLOTS, SLOTS), bool), k=1), v, NO_PAIR)


def best_pair(d):
    """(delta, a, b, tied): the least delta, ties to the least a, then the least b."""
    flat = int(np.argmin(d))                   # row-major first minimum: least a, then least b
    a, b = divmod(flat, SLOTS)
    return int(d[a, b]), a, b, int((d == d[a, b]).sum()) > 1


def descend(inst, slot, max_passes, deltas=deltas_table, log=None):
    """(new row, gain, passes, perm); log (a list) receives (delta, a, b, tied) per applied pass."""
    row = np.asarray(slot).copy()
    perm = np.arange(SLOTS, dtype=np.uint8)
    if row.max(initial=0) >= SLOTS:
        return row, 0, 0, perm
    gain = passes = 0
    while passes < max_passes:
        dl, a, b, tied = best_pair(deltas(inst, row))
        if dl >= 0:
            break
        row = swapped(row, a, b)
        perm = swapped(perm, a, b)
        gain -= dl
        passes += 1
        if log is not None:
            log.append((dl, a, b, tied))
    return row, gain, passes, perm


def prefix(slot, log, k):
    """descend(inst, slot, k) from the log of a longer descent of the same row: the
    descent is deterministic, so a capped one is a prefix of the uncapped one."""
    row, perm, gain = np.asarray(slot).copy(), np.arange(SLOTS, dtype=np.uint8), 0
    for dl, a, b, _ in log[:k]:
        row, perm, gain = swapped(row, a, b), swapped(perm, a, b), gain - dl
    return row, gain, min(k, len(log)), perm


def stack(out):
    """A list of (row, gain, passes, perm) as four arrays."""
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.int32), np.stack([o[3] for o in out]))


def descend_rows(inst, slots, max_passes, deltas=deltas_table):
    return stack([descend(inst, r, max_passes, deltas) for r in slots])
