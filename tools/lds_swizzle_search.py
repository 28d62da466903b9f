import itertools
groups = [list(range(0,4))+list(range(12,16))+list(range(20,28)), list(range(4,12))+list(range(16,20))+list(range(28,32)),
          list(range(32,36))+list(range(44,48))+list(range(52,60)), list(range(36,44))+list(range(48,52))+list(range(60,64))]
# write groups for ds_write_b128: 8 x 8 contiguous lanes
wgroups = [list(range(8*i, 8*i+8)) for i in range(8)]
def worst_read(RB, UPL, sw):
    UR = RB//16
    KB = max(UR//(4*UPL),1)
    worst = 0
    for s in range(KB):
        for h in range(UPL):
            for g in groups:
                slots = {}
                for lane in g:
                    r, q = lane & 15, lane >> 4
                    unit = (4*s+q)*UPL + h
                    a = r*RB + (((unit ^ sw(r)) & (UR-1)) << 4)
                    slots.setdefault((a % 256)//16, set()).add(a)
                worst = max(worst, max(len(v) for v in slots.values()))
    return worst
def lin(mat, nb):   # mat: list of nb 4-bit masks
    def f(r):
        v = 0
        for b, m in enumerate(mat):
            v |= (bin(r & m).count("1") & 1) << b
        return v
    return f
for RB, UPL in ((128,1),(128,2),(64,1)):
    nb = 3 if RB == 128 else 2
    best = None
    for mat in itertools.product(range(16), repeat=nb):
        w = worst_read(RB, UPL, lin(mat, nb))
        if best is None or w < best[0]:
            best = (w, mat)
            if w == 1: break
    print(RB, UPL, best)
print("verify:")
print(worst_read(128,1,lambda r:(r>>1)&7), worst_read(128,2,lambda r:((r>>1)&1)|(r&4)), worst_read(64,1,lambda r:((r>>2)&1)<<1))

# ---- "rc64": the REAL operand of the mixed fp64 x complex128 kernel (gett_gen_rc64.inc) -------------------------------------------
# 8-byte elements at K-tile 8 = 64-byte rows (4 units), one 16-byte unit per lane: lane (r, q) reads unit q of row r — the read pattern
# of the (64, 1) case above.  Beside the read, the staging writes of its four (orientation, V) maps (GenUnitMap<ORIENT, 64, 8, V, 256>)
# under each candidate: ds_write_b128 (K-contiguous, V = 2: 8 x 8 contiguous lanes) and ds_write_b64 (the others: 4 x 16 contiguous
# lanes), banks (address / 4) mod 32.  Worst number of distinct addresses of one group on one bank = cycles the group takes.
def rc64_addr(row, k, sw):
    kb = k * 8
    return row * 64 + ((((kb >> 4) ^ sw(row)) & 3) << 4) + (kb & 15)
def rc64_worst_write(orient, V, sw):
    ROWS, BK, T = 64, 8, 256
    KV, TPK = BK // V, T // BK
    NU = ROWS * BK // (V * T)
    worst = 0
    wide = orient == 1 and V == 2                  # one 16-byte store per unit; else one 8-byte store per element
    glen = 8 if wide else 16
    for i in range(NU):
        for e in range(1 if wide else V):
            for wave in range(4):
                for g0 in range(0, 64, glen):
                    banks = {}
                    for lane in range(g0, g0 + glen):
                        tid = wave * 64 + lane
                        if orient:
                            row, k = tid // KV + i * (T // KV), (tid % KV) * V
                        else:
                            row, k = ((tid % TPK) + i * TPK) * V + e, tid // TPK
                        a = rc64_addr(row, k, sw)
                        for d in range(4 if wide else 2):
                            banks.setdefault(((a >> 2) + d) % 32, set()).add(a)
                    worst = max(worst, max(len(v) for v in banks.values()))
    return worst
print("rc64 (real fp64 operand, 64-byte rows, one unit per lane): (read, writes F/V2, F/V1, K/V2, K/V1) per swizzle")
rows = []
for mat in itertools.product(range(16), repeat=2):
    f = lin(mat, 2)
    rows.append((worst_read(64, 1, f), tuple(rc64_worst_write(o, v, f) for o, v in ((0, 2), (0, 1), (1, 2), (1, 1))), mat))
rows.sort(key=lambda t: (t[0], sum(t[1]), t[2]))
print("best:", rows[0])
own = lambda r: (r >> 1) & 3
print("GenImageR64's (row >> 1) & 3:", worst_read(64, 1, own), tuple(rc64_worst_write(o, v, own) for o, v in ((0, 2), (0, 1), (1, 2), (1, 1))))
fam = lambda r: ((r >> 2) & 1) << 1
print("the family's 64-byte-row swizzle ((row >> 2) & 1) << 1:", worst_read(64, 1, fam), tuple(rc64_worst_write(o, v, fam) for o, v in ((0, 2), (0, 1), (1, 2), (1, 1))))
none = lambda r: 0
print("no swizzle:", worst_read(64, 1, none), tuple(rc64_worst_write(o, v, none) for o, v in ((0, 2), (0, 1), (1, 2), (1, 1))))
