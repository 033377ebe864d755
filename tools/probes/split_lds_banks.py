"""LDS bank conflicts of the permuted phases of k_copy_split.h, enumerated on the host (no GPU) with the MI355X's
per-instruction lane groups:

  ds_write_b128        eight groups of 8 consecutive lanes, bank = (address / 4) mod 32: the 16-byte slot is position mod 8
  single elements      (ds_write_b16 / b8, ds_read_u16 / u8) two groups of 32 lanes, bank = (address / 4) mod 32; lanes on
                       one dword are one address
  (the linear phases -- lane = position, ds_read_b128 / ds_write_b128 -- are conflict free by construction)

for every head size D up to 512, both element sizes and the three tile lengths, with the image positions of the kernel:

  Pg(w, g) = w * NG + (g + rot(w)) mod NG,  rot(w) = (NG even ? w : 0) + w / 8        (row image)
  Ps(g, w) = g * TT + (w + g) mod TT                                                   (split image, K scatter)

Prints, per phase, how many geometries are N-way at worst, and lists those above two-way.

    python tools/probes/split_lds_banks.py
"""


def worst(groups, positions, mod):
    w = 0
    for grp in groups:
        by = {}
        for lane in grp:
            p = positions[lane]
            if p is not None:
                by.setdefault(p % mod, set()).add(p)
        w = max([w] + [len(v) for v in by.values()])
    return w


W128 = [list(range(i, i + 8)) for i in range(0, 64, 8)]
H32 = [list(range(32)), list(range(32, 64))]


def Pg(w, g, NG):
    return w * NG + (g + (w if NG % 2 == 0 else 0) + (w >> 3)) % NG


def Ps(g, w, TT):
    return g * TT + (w + g) % TT


def main(min_ng=4):
    res = {}
    for eb in (2, 1):
        X = 16 // eb
        for TT in (8, 16, 32):
            for D in range(X * min_ng, 513, X):
                NG = D // X
                NV = TT * NG
                if NV * 16 > 16384:  # SPLIT_MAX_IMAGE
                    continue
                kg = ks = vv = 0
                for v0 in range(0, NV, 64):
                    lanes = range(v0, v0 + 64)
                    kg = max(kg, worst(W128, [Pg(v % TT, v // TT, NG) if v < NV else None for v in lanes], 8))
                    ks = max(ks, worst(W128, [Ps(v % NG, v // NG, TT) if v < NV else None for v in lanes], 8))
                res.setdefault(("K gather: split-side ds_write_b128 into the row image", kg), []).append((eb, TT, D))
                res.setdefault(("K scatter: row-side ds_write_b128 into the split image", ks), []).append((eb, TT, D))
                if TT < X:
                    continue  # V has no 16-byte run there: element path
                GPR = TT // X
                for v0 in range(0, NV, 64):
                    for k in range(X):
                        dwords = []
                        for v in range(v0, v0 + 64):
                            if v >= NV:
                                dwords.append(None)
                                continue
                            d, part = v // GPR, v % GPR
                            dwords.append((Pg(part * X + k, d // X, NG) * 16 + (d % X) * eb) // 4)
                        vv = max(vv, worst(H32, dwords, 32))
                res.setdefault(("V gather / scatter: split-side single elements of the row image", vv), []).append((eb, TT, D))
    for key in sorted(res):
        geoms = res[key]
        print(f"{key[0]}: {key[1]}-way at worst for {len(geoms)} geometries" +
              (f": (element bytes, TT, D) = {geoms}" if key[1] > 2 else ""))
    return max(k[1] for k in res)


if __name__ == "__main__":
    raise SystemExit(0 if main() <= 2 else 1)
