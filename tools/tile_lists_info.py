#!/usr/bin/env python3
"""The position slots of bench.py's tree (pfq_tile_lists_info): columns with slots, their bytes, and the tiles one step of
bench.py's reads took from slots / loaded dense.  usage: tools/tile_lists_info.py [leaves] [reads]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from phagefilter_amd import BloomTree, _ffi
    n_g = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 8 * 1024 * 1024
    glen, rl = 50000, 150
    L, dev = _ffi.lib(), torch.device("cuda:0")
    genomes = torch.empty(n_g * glen, dtype=torch.uint8, device=dev)
    _ffi.check(L.pfq_synth_genomes_device(genomes.data_ptr(), n_g, glen, bench.GENOME_SEED, None))
    tree = BloomTree.build_balanced_device(genomes.data_ptr(), glen, n_g, [f"G{i:05d}" for i in range(n_g)], bench.K, bench.NBITS,
                                           bench.NUM_HASHES, bench.SEEDS[0], bench.SEEDS[1], 0.001, 5000000, device=0)
    reads = torch.empty(B * rl + 64, dtype=torch.uint8, device=dev)
    _ffi.check(L.pfq_synth_reads_device(reads.data_ptr(), 0, B, rl, genomes.data_ptr(), glen, n_g, bench.READ_SEED, None))
    off = torch.arange(B + 1, dtype=torch.int64, device=dev) * rl
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = tree.tile_lists_info()          # builds the layout, the slots with it
    layout_s = time.perf_counter() - t0
    tree.query_device(reads.data_ptr(), off.data_ptr(), B, B * rl, 1.0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    info = tree.tile_lists_info()
    st = tree.last_stats()
    print(json.dumps({"leaves": n_g, "reads": B, "layout_seconds": layout_s, "tile_mode": int(st.tile_mode), **info}))
    tree.close()


if __name__ == "__main__":
    main()
