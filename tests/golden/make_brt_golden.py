"""Record tests/golden/brt_ranges.json from the REFERENCE's range tree itself.

The reference's lib/brtree.c (brt_add, brt_loop_on_ranges) is compiled in a
temporary directory behind a stub lib.h written here, with a driver written
here that inserts each input set in its given order, walks the tree and folds
the walk as gc_data_stat_cb does (mdsl/gc.c:746-753: valid += high - low, max
= the largest high).  Nothing of the reference enters the repository: only
the input sets and what its tree answered.

About 200 sets of 1 ... 28 ranges: random dense and sparse ones, and the
directed kinds named in KINDS.  No set holds a range with high <= low: the
tree's comparator is inconsistent on such a node.

  python tests/golden/make_brt_golden.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

STUB_LIB_H = r"""
#ifndef STUB_LIB_H
#define STUB_LIB_H
#define _GNU_SOURCE
#include <errno.h>
#include <search.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef uint64_t u64;
struct brtnode { u64 low, high; };
#define xfree free
#define hvfs_err(module, ...) fprintf(stderr, __VA_ARGS__)
int brt_add(struct brtnode *n, void **rootp);
void brt_destroy(void *root, void (*free_node)(void *p));
int brt_loop_on_ranges(void **rootp, void *arg, void (*cb)(u64 low, u64 high, void *arg));
#endif
"""

DRIVER_C = r"""
#include "lib.h"
struct fold { u64 valid, max, n; u64 out[256]; };
static void on_range(u64 low, u64 high, void *arg)
{
    struct fold *f = arg;
    f->valid += high - low;
    if (high > f->max)
        f->max = high;
    f->out[2 * f->n] = low;
    f->out[2 * f->n + 1] = high;
    f->n++;
}
int main(void)
{
    unsigned n;
    while (scanf("%u", &n) == 1) {
        void *root = NULL;
        struct fold f = {0};
        for (unsigned i = 0; i < n; i++) {
            struct brtnode *p = malloc(sizeof(*p));
            unsigned long long lo, hi;
            if (scanf("%llu %llu", &lo, &hi) != 2)
                return 2;
            p->low = lo;
            p->high = hi;
            brt_add(p, &root);
        }
        brt_loop_on_ranges(&root, &f, on_range);
        printf("%llu %llu %llu", (unsigned long long)f.n, (unsigned long long)f.valid, (unsigned long long)f.max);
        for (u64 k = 0; k < 2 * f.n; k++)
            printf(" %llu", (unsigned long long)f.out[k]);
        printf("\n");
        brt_destroy(root, free);
    }
    return 0;
}
"""

KINDS = ("touching", "gap_of_one", "nested", "identical", "one_covers_all", "descending", "equal_low")


def directed(kind: str, rng: random.Random):
    n = rng.randint(2, 28)
    base = rng.choice([0, 7, 1 << 20, 1 << 39])
    if kind == "touching":
        r = [(base + 10 * i, base + 10 * i + 10) for i in range(n)]
    elif kind == "gap_of_one":
        r = [(base + 10 * i, base + 10 * i + 9) for i in range(n)]
    elif kind == "nested":
        r = [(base + i, base + 200 - i) for i in range(n)]
    elif kind == "identical":
        r = [(base + 5, base + 50)] * n
    elif kind == "one_covers_all":
        r = [(base + 10 * i + 1, base + 10 * i + 4) for i in range(n)]
        r.insert(rng.randrange(n + 1), (base, base + 10 * n + 5))
    elif kind == "descending":
        r = [(base + 6 * i, base + 6 * i + rng.randint(1, 9)) for i in reversed(range(n))]
        return r
    else:                                               # equal low, different high
        r = [(base + 100 * (i % 3), base + 100 * (i % 3) + 1 + rng.randint(0, 120)) for i in range(n)]
    if kind not in ("one_covers_all",):
        rng.shuffle(r)
    return r


def random_set(rng: random.Random, dense: bool):
    n = rng.randint(1, 28)
    span = 50 if dense else 1 << 38
    out = []
    for _ in range(n):
        lo = rng.randrange(span)
        out.append((lo, lo + 1 + rng.randrange(12 if dense else 1 << rng.randint(1, 28))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "brt_ranges.json"))
    args = ap.parse_args()
    rng = random.Random(0xB27)
    sets = []
    for kind in KINDS:
        for _ in range(8):
            sets.append((kind, directed(kind, rng)))
    for i in range(144):
        sets.append(("dense" if i % 2 == 0 else "sparse", random_set(rng, i % 2 == 0)))
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "lib.h"), "w") as f:
            f.write(STUB_LIB_H)
        with open(os.path.join(tmp, "driver.c"), "w") as f:
            f.write(DRIVER_C)
        # a copy beside the stub: #include "lib.h" looks in the including file's directory first
        shutil.copy(os.path.join(args.reference, "lib", "brtree.c"), os.path.join(tmp, "brtree.c"))
        exe = os.path.join(tmp, "brt_driver")
        subprocess.run(["gcc", "-O1", "-w", "-I", tmp, "-o", exe, os.path.join(tmp, "driver.c"),
                        os.path.join(tmp, "brtree.c")], check=True)
        text = "".join(f"{len(r)} " + " ".join(f"{lo} {hi}" for lo, hi in r) + "\n" for _, r in sets)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(sets)
    cases = []
    for (kind, r), line in zip(sets, lines):
        v = [int(x) for x in line.split()]
        n, valid, mx, flat = v[0], v[1], v[2], v[3:]
        assert len(flat) == 2 * n
        cases.append({"kind": kind, "in": [x for lo_hi in r for x in lo_hi], "out": flat, "valid": valid, "max": mx})
    with open(args.out, "w") as f:
        json.dump({"generator": "tests/golden/make_brt_golden.py",
                   "reference": "lib/brtree.c brt_add, brt_loop_on_ranges; mdsl/gc.c:746-753 gc_data_stat_cb",
                   "layout": "in, out: flat low, high pairs", "cases": cases}, f, separators=(",", ":"))
    print(f"{len(cases)} sets -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
