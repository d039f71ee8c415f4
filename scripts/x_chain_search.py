"""Search for a short signed chain for the BN parameter x (curve.h BN_X_CHAIN; 62 squarings + 13 products over {1, 17, 35} before
this search, 62 + 12 since) in the space the chain interpreter really allows: any RUNNING VALUE may be parked and used as a
later multiplier, its negative is free (a conjugate / a negated point) but takes a slot of its own, and a parked value may be loaded as a new start.

  prefix   forward, exhaustive: from 1, up to PREFIX products r <- r 2^s + d (d = 1 or a parked signed value, optional load of a
           parked value first), every value below 2^BITS; each new value may be parked as +r, -r, both or not, and -1 may be
           parked at the start; at most SLOTS - 1 parked values besides the input.
  main     backward from x: x' = (x - d) >> tz(x - d) for every signed d of the dictionary (running values are odd, so the shift
           is the whole run of zeros), layer by layer, keeping the BEAM smallest values of a layer; a layer that contains the
           prefix's end value or a parked positive value (a load) closes a chain.
A chain counts when it has <= MAX_PRODUCTS products, <= MAX_SQUARINGS squarings and <= SLOTS slots.  The backward part is a
beam search, not an exhaustive one: "none found" is a statement about this search (its parameters are printed), not a proof.
Usage: python scripts/x_chain_search.py [--prefix 2] [--bits 12] [--beam 4000] [--products 12] [--jobs 8]
The chain in curve.h is the first result of --prefix 3 --bits 12 --beam 1000 (449 k dictionaries, about three minutes on eight
cores); --prefix 2 finds none with 12 products, --products 13 --bits 8 finds the chain over {1, 17, 35} again."""
import argparse
import multiprocessing
import time

import numpy as np

X = 0x44e992b44a6909f1
SLOTS = 5
MAX_SQUARINGS = 64


def prefixes(max_products, bits):
    """{signed dictionary (sorted tuple, without +1): {end value: (products, squarings, steps)}}, cheapest build per end value"""
    lim = 1 << bits
    out = {}

    def visit(r, parked, products, sq, steps):
        key = tuple(sorted(parked))
        ends = out.setdefault(key, {})
        # the main chain may continue from r or load any parked positive value (or the input)
        for end in {r, 1} | {v for v in parked if v > 0}:
            if end not in ends or ends[end][:2] > (products, sq):
                ends[end] = (products, sq, steps)
        if products == max_products:
            return
        starts = {r} | {v for v in parked if v > 0} | {1}
        for start in starts:
            for s in range(1, bits):
                base = start << s
                if base >= 2 * lim:
                    break
                for d in (1,) + parked:
                    v = base + d
                    if v <= 1 or v >= lim or v == start:
                        continue
                    room = SLOTS - 1 - len(parked)
                    for add in ((), (v,), (-v,), (v, -v)):
                        if len(add) > room or any(a in parked for a in add):
                            continue
                        visit(v, parked + add, products + 1, sq + s, steps + ((start, s, d, add),))

    visit(1, (), 0, 0, ())
    visit(1, (-1,), 0, 0, ())
    return out


def backward(dic, ends, max_products, beam):
    """chains for one dictionary: [(products, squarings, end, [(d, shift), ...])]"""
    S = np.array((1,) + dic, dtype=np.int64)
    budget = max_products - min(p for p, _, _ in ends.values())
    targets = np.array(sorted(ends), dtype=np.int64)
    layers = []                                       # per layer: values, parent index, d index, shift
    vals = np.array([X], dtype=np.int64)
    found = []
    for k in range(1, budget + 1):
        c = (vals[:, None] - S[None, :]).ravel()
        par = np.repeat(np.arange(vals.size), S.size)
        di = np.tile(np.arange(S.size), vals.size)
        ok = c > 0
        c, par, di = c[ok], par[ok], di[ok]
        if c.size == 0:
            break
        low = c & -c
        sh = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
        ok = sh >= 1                                  # r 2^0 + d would be even: not a running value
        c, par, di, sh = c[ok] >> sh[ok], par[ok], di[ok], sh[ok]
        c, first = np.unique(c, return_index=True)
        par, di, sh = par[first], di[first], sh[first]
        if c.size > beam:
            c, par, di, sh = c[:beam], par[:beam], di[:beam], sh[:beam]       # np.unique sorts: the smallest
        layers.append((c, par, di, sh))
        hit = np.nonzero(np.isin(c, targets))[0]
        for h in hit:
            end = int(c[h])
            p0, s0, _ = ends[end]
            if k + p0 > max_products:
                continue
            path, i = [], int(h)
            for lv in range(len(layers) - 1, -1, -1):
                cc, pp, dd, ss = layers[lv]
                path.append((int(S[dd[i]]), int(ss[i])))
                i = int(pp[i])
            path.reverse()                            # from x downwards; applied in reverse when run forwards
            sq = s0 + sum(s for _, s in path)
            if sq <= MAX_SQUARINGS:
                found.append((k + p0, sq, end, path))
        vals = c
    return found


def replay(end, path):
    r = end
    for d, s in reversed(path):
        r = (r << s) + d
    return r


def work(args):
    dic, ends, max_products, beam = args
    return dic, backward(dic, ends, max_products, beam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", type=int, default=2)
    ap.add_argument("--bits", type=int, default=12)
    ap.add_argument("--beam", type=int, default=4000)
    ap.add_argument("--products", type=int, default=12)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    t0 = time.time()
    pre = prefixes(a.prefix, a.bits)
    print("prefixes of up to %d products, values below 2^%d: %d dictionaries (%.0f s)" % (a.prefix, a.bits, len(pre), time.time() - t0), flush=True)
    jobs = [(dic, ends, a.products, a.beam) for dic, ends in pre.items()]
    best = []
    with multiprocessing.Pool(a.jobs) as pool:
        for n, (dic, found) in enumerate(pool.imap_unordered(work, jobs, chunksize=16)):
            for products, sq, end, path in found:
                assert replay(end, path) == X
                best.append((products, sq, dic, end, path))
            if n % 2000 == 0:
                print("  %d / %d dictionaries, %d chains so far (%.0f s)" % (n, len(jobs), len(best), time.time() - t0), flush=True)
    best.sort(key=lambda b: (b[0], b[1], len(b[2])))
    print("search: prefix <= %d products, parked values < 2^%d, beam %d, <= %d products, <= %d squarings, <= %d slots: %d chains"
          % (a.prefix, a.bits, a.beam, a.products, MAX_SQUARINGS, SLOTS, len(best)))
    for products, sq, dic, end, path in best[:10]:
        build = pre[dic][end][2]
        print("%d products + %d squarings, parked %s; build %s; from %d: %s" % (products, sq, list(dic), list(build), end,
                                                                              " ".join("<<%d%+d" % (s, d) for d, s in reversed(path))))
    if not best:
        print("none found")


if __name__ == "__main__":
    main()
