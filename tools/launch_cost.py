#!/usr/bin/env python3
"""Host cost of one learner launch through the facade, on one MI355X: the mean wall time of a one-step `vec.td_run(1)` and of a
one-step `vec.tree_search_run(1, simulations=1, tree_depth=1, depth=0)` at N = 64 on the default 4 x 4 grid, where the kernel is
next to nothing and what is measured is Python, the argument checks and the library's entry points; and the cost of one
`engine.stores()` call alone.  Prints one JSON line.
Usage: python tools/launch_cost.py [--launches 10000] [--queries 100000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import griduniverse_amd as gua  # noqa: E402


def mean_us(fn, n, sync):
    for _ in range(max(n // 50, 10)):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=10000)
    ap.add_argument('--queries', type=int, default=100000)
    a = ap.parse_args()
    vec = gua.VecGridUniverse(64, seed=0)
    try:
        vec.reset()
        out = {'td_run_us': mean_us(lambda: vec.td_run(1), a.launches, vec.engine.sync),
               'tree_search_run_us': mean_us(lambda: vec.tree_search_run(1, simulations=1, tree_depth=1, depth=0), a.launches, vec.engine.sync)}
        if hasattr(vec.engine, 'stores'):
            out['stores_us'] = mean_us(vec.engine.stores, a.queries, vec.engine.sync)
    finally:
        vec.close()
    print(json.dumps({k: round(v, 3) for k, v in out.items()}))


if __name__ == '__main__':
    main()
