"""The oracle's side of one long-lived tree driven through every entry point (tests/test_gpu_mixed_sequences.py), without a device.

TreeModel extends the Model of tests/test_gpu_call_sequences.py to everything a pfq_tree carries from call to call: the leaf
totals and the delta base, the clade, taxon, abundance, coverage and sweep accumulators, the results of the last call and
whether each is still valid, the block parsed last and the block prepared last, whether pfq_text_format is valid, and the
settings that live on the tree.  Every expectation comes from the oracle and the *_ref modules; the lifetime rules are those of
include/pfq.h, applied literally.

Since the depletion (pfq_prep_deplete) involves two trees, a Play runs two: the main tree and beside it, for the whole deck, the
screen — a second TreeModel with its own k, hashes, size and seeds — which prepared blocks are depleted against and which is
queried, parsed for and grown on its own.  A depletion that is not refused is a query call on the screen and on the screen alone.

deck() is the schedule: per seed a shuffled deck that holds every operation at least twice, patched so that every pair of
PAIRS occurs.  Play runs a deck: the model side always, the device side when it is given one, compared call by call.
tests/test_mixed_model_cpu.py runs it without a device."""
import ctypes as C

import numpy as np

import abund_ref
import adapter_ref
import cluster_ref
import correct_ref
import cover_ref
import deplete_ref
import format_cases as fc
import format_ref
import frames_ref
import overlap_ref
import prep_ref
import sim_ref
import sweep_ref
import tax_ref
import text_ref
from oracle import pfq_oracle as orc
from phagefilter_amd import PfqError, _ffi, pack_reads
from test_gpu_call_sequences import K, THRESHOLDS, Model, check_counts, workload
from test_gpu_capacity import close_families
from test_gpu_frames import GRID
from test_gpu_lca import Clades, best_sets, csr_of, oracle_sets, pair_scores
from test_gpu_paired import combine, mate_sets
from test_gpu_parity import RNG, oracle_tree, rand_dna
from test_gpu_prep import pack_quals
from test_gpu_regimes import mutate
from test_gpu_scores import Contains, expected_scores
from test_gpu_tax import random_taxonomy

PFQ_ERR_ARG, PFQ_ERR_UNSUPPORTED, PFQ_ERR_STATE = -1, -4, -6
NO = 0xFFFFFFFF
SMALL = 72                                   # units of a call whose scores, best rows, coverage and sweep are worked out in Python
AD33 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
AD2 = b"CTGTCTCTTATACACATCT"
ADAPTER_SETS = (((AD33,), (), 5, 10), ((AD33, AD2), (AD2,), 8, 20), None)
OVERLAPS = ((30, 10), (12, 50), None)
CORRECTS = ((30, 14), (35, 5), None)         # (high, low) of the mate correction
Q_HIGH, Q_LOW = 40 + 33, 2 + 33              # planted qualities: at least every `high`, at most every `low` of CORRECTS
# the screen of each deck: its own k (above the main tree's, so a read the trimmer keeps can still lie under it), hashes, size, seeds
SCREEN_BALANCED = dict(k=25, nbits=100003, h=3, seeds=(0x1111222233334444, 0x9999AAAABBBBCCCC))
SCREEN_GREEDY = dict(k=23, fpr=0.001, largest=5000, seeds=(11, 13))
UNDER_K = 22                                 # K <= UNDER_K < both screens' k
SWEEP_LISTS = ((0.3, 0.7, 1.0), (0.7, 0.9), None)
PREP_PARAMS = ({}, dict(trim_quality=20, trim_window=4, poly_x=10, min_length=K),
               dict(trim_quality=20, trim_window=4, poly_x=10, min_length=K, max_n=3, min_complexity=30))
KNOBS = (("PFQ_TILE_LISTS", "0"), ("PFQ_ENTRY_PACK", "0"), ("PFQ_ENTRY_PACK", "2"), ("PFQ_TILE_STREAM", "0"), ("PFQ_BLOCK", "0"), ("PFQ_BLOCK", "1"),
         ("PFQ_BATCH_EMIT", "0"), ("PFQ_BATCH_EMIT", "1"), ("PFQ_SPLIT_RECORDS", "0"), ("PFQ_SPLIT_RECORDS", "1"), ("PFQ_FMT_GRID", "1"),
         ("PFQ_FMT_HASH_BITS", "2"), ("PFQ_FRAME_PIECE", "64"), ("PFQ_SWEEP_LDS", "0"), ("PFQ_SIM_SLICES", "7"))

# ---------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------
QUERY_OPS = ("host", "dev", "text", "prepq", "frames", "frames_dev")
BLOCK_OPS = ("parse", "prep", "prep_paired")
NOTHING_OPS = ("format", "readout", "similarity", "recluster", "option", "delta")
STATE_OPS = ("reset_counts", "abundance_reset", "coverage_reset", "sweep_reset", "set_sweep", "set_taxonomy", "set_adapters", "set_mate_overlap",
             "set_mate_correct")
SCREEN_OPS = ("deplete", "screen_query")     # the two calls that involve the second tree
OPS = QUERY_OPS + BLOCK_OPS + NOTHING_OPS + STATE_OPS + SCREEN_OPS + ("refuse",)
# adjacent operations every deck must hold; an entry is (operation, forced result mode or None)
PAIRS = {
    "query -> format": [("text", "hits"), ("format", None)],
    "frames -> format": [("frames", None), ("format", None)],
    "prep-query -> format": [("prepq", "hits"), ("format", None)],
    "parse -> parse -> query": [("parse", None), ("parse", None), ("text", None)],
    "prep -> prep -> query": [("prep", None), ("prep", None), ("prepq", None)],
    "counts-only -> non-query -> counts-only": [("host", "counts"), ("parse", None), ("dev", "counts")],
    "host query -> text parse -> host query": [("host", None), ("parse", None), ("host", None)],
    # the depletion (pfq_prep_deplete).  A deplete "again" repeats the call before it, which then removes nothing; "first", "either"
    # and "both" draw a threshold above 0 (at 0 every unit goes), the latter two force the pair mode; prep_paired "quals": with qualities
    "prep -> deplete -> prepq": [("prep", None), ("deplete", None), ("prepq", None)],
    "prep_paired -> deplete -> prepq": [("prep_paired", None), ("deplete", "both"), ("prepq", None)],
    "prep -> deplete -> deplete -> prepq": [("prep", None), ("deplete", "first"), ("deplete", "again"), ("prepq", None)],
    # the depleted block's own classification is still queued (the wait for pp_free[slot])
    "prep -> prepq(counts) -> deplete -> prepq(hits)": [("prep", None), ("prepq", "counts"), ("deplete", None), ("prepq", "hits")],
    # the previous block's classification is queued on the other CSR set
    "prep -> prepq(counts) -> prep -> deplete -> prepq(counts)": [("prep", None), ("prepq", "counts"), ("prep", None), ("deplete", None), ("prepq", "counts")],
    "screen_query(hits) -> deplete": [("screen_query", "hits"), ("deplete", None)],
    "text(hits) -> prep -> deplete -> format": [("text", "hits"), ("prep", None), ("deplete", None), ("format", None)],
    "overlap, adapters, correction -> prep_paired -> deplete -> prepq": [("set_mate_overlap", "on"), ("set_adapters", "on"), ("set_mate_correct", "on"),
                                                                         ("prep_paired", "quals"), ("deplete", "either"), ("prepq", None)],
    # once per deck the screen's own parse_text / query_text / format_text, valid when the depletion comes
    "screen text -> prep -> deplete": [("screen_query", "text"), ("prep", None), ("deplete", None)],
}
DEPLETE_RUNS = [name for name in PAIRS if "deplete" in name]


# on the greedy tree: a block parsed and a block prepared before the topology changes, queried after it against the new leaves
STALE_INSERT = [("parse", None), ("prep", None), ("insert", None), ("text", "hits"), ("prepq", "hits")]
STALE_PRUNE = [("parse", None), ("prep", None), ("prune", None), ("text", "hits"), ("prepq", "hits")]
# ... and a prepared block depleted when it is older than the main tree's leaves, or than the screen's
DEPLETE_INSERT = [("prep", None), ("insert", None), ("deplete", None), ("prepq", "hits")]
DEPLETE_PRUNE = [("prep", None), ("prune", None), ("deplete", None), ("prepq", "hits")]
DEPLETE_SCREEN_INSERT = [("prep", None), ("screen_insert", None), ("deplete", None), ("prepq", "hits")]
GREEDY_RUNS = (STALE_INSERT, STALE_PRUNE, DEPLETE_INSERT, DEPLETE_PRUNE, DEPLETE_SCREEN_INSERT)


def has_run(deck, run):
    """Whether `run` occurs in `deck` as adjacent entries; a forced mode must be the deck's, an operation alone matches any."""
    def fits(entry, want):
        return entry[0] == want[0] and (want[1] is None or entry[1] == want[1])
    return any(all(fits(deck[i + j], w) for j, w in enumerate(run)) for i in range(len(deck) - len(run) + 1))


def deck(seed, greedy=False, repeats=2):
    """The schedule of one seed: every operation `repeats` times (the queries of a parsed or prepared block come once more behind
    their block and once more on their own, which repeats the query) and the depletion runs of PAIRS as units of their own,
    shuffled, then every run of PAIRS that the shuffle did not produce appended.  On the greedy tree two insertions lie in the
    middle and two prunes near the end, each followed once by queries of the older blocks and once by a depletion of the older
    prepared block, and the screen takes its spare genome between a prep and its depletion."""
    rng = np.random.default_rng(seed)
    units = []
    for op in OPS:
        units += [[(op, None)]] * repeats
    units += [[("parse", None), ("text", None)]] * repeats + [[("prep", None), ("prepq", None)]] * repeats
    units += [[("prep_paired", None), ("prepq", None)]] * repeats + [[("text", "hits"), ("format", None), ("format", None)]]
    units += [[("host", "counts"), ("dev", "counts"), ("dev", "counts")], [("set_sweep", "on"), ("host", "scores")], [("set_taxonomy", None), ("dev", "hits")]]
    units += [[("set_mate_overlap", "on"), ("set_adapters", "on"), ("prep_paired", None), ("prepq", None)]]
    units += [[("parse", "even"), ("text", "paired"), ("format", None)]]      # (fragments: a successful query_text that leaves format_text invalid)
    units += [list(PAIRS[name]) for name in DEPLETE_RUNS]
    if greedy:                                      # the screen grows by a leaf between a prep and its depletion, once
        units += [list(DEPLETE_SCREEN_INSERT)]
    units = [units[i] for i in rng.permutation(len(units))]
    if greedy:                                      # (whole units: no run that belongs together is split)
        mid = len(units) // 2
        after = [("readout", None), ("parse", None)]
        units = (units[:mid] + [STALE_INSERT + after + DEPLETE_INSERT + [("text", "hits")]] + units[mid:-3] +
                 [STALE_PRUNE + after + [("prep", None), ("prune", "deeper")] + DEPLETE_PRUNE[2:] + [("text", "hits"), ("readout", None)]] + units[-3:])
    out = [e for u in units for e in u]
    for run in PAIRS.values():
        if not has_run(out, run):
            out += run
    return out


def coverage_of(d):
    """(operations and how often each occurs, the runs of PAIRS that are missing)."""
    count = {op: sum(1 for e in d if e[0] == op) for op in OPS}
    return count, [name for name, run in PAIRS.items() if not has_run(d, run)]


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def rows_of(sets):
    return [sorted(s) for s in sets]


class TreeModel(Model):
    def __init__(self, ot):
        super().__init__(ot)
        self.adapters = None        # (set1, set2, O, E)
        self.overlap = None         # (O, E)
        self.correct = None         # (high, low)
        self.sweep_list = None
        self.text = None            # the block parsed last: dict(recs, reads, fastq, scan)
        self.prep = None            # the block prepared last: dict(want, paired)
        self.seen = {}              # what the expectations held, for the non-vacuity conditions
        self.new_leaves()

    # ---- what follows the leaves (pfq.h: pfq_tree_prune and pfq_tree_insert)
    def new_leaves(self):
        for block in (self.text, self.prep):                               # the blocks are sequence data: they stay, and are older than the leaves now
            if block is not None:
                block["stale"] = True
        names = self.names()
        self.n_leaves = len(names)
        self.total = {t: self.total.get(t, 0) for t in names}
        self.base = {t: self.base.get(t, 0) for t in names}
        self.cm = Clades(self.ot)
        self.contains = Contains(self.ot)
        self.clade_here = np.zeros(len(self.cm.nodes), dtype=np.uint64)     # zeroed
        self.tax = self.nodes = self.tax_here = self.tax_any = None        # the taxonomy is dropped
        self.abundance_reset()                                              # the log and the sketch are cleared
        self.coverage_reset(same_leaves=False)
        self.sweep_reset()                                                  # zeroed and made for the new leaves, the list stays
        self.fmt_valid = False
        if not hasattr(self, "last"):
            self.last = dict(lca=None, taxa=None, best=None, scores=None)   # (what the last call left stays until the next query call)

    def note(self, key, cond=True):
        if cond:
            self.seen[key] = self.seen.get(key, 0) + 1

    # ---- resets
    def reset(self):                # pfq_leaf_counts_reset
        super().reset()
        self.clade_here[:] = 0
        if self.nodes is not None:
            self.tax_here[:] = 0
            self.tax_any[:] = 0
        self.abundance_reset()
        self.coverage_reset()
        self.sweep_reset()

    def abundance_reset(self):
        self.log = abund_ref.classify([], self.n_leaves)
        self.log_ok = True

    def coverage_reset(self, same_leaves=True):
        """An empty sketch; the oracle's answers per (leaf, k-mer) are kept while the leaves are the same."""
        self.sketcher = cover_ref.TreeSketcher(self.ot, share=self.sketcher if same_leaves else None)

    def sweep_reset(self):
        T, L = len(self.sweep_list or ()), self.n_leaves
        self.sw = {"pass": np.zeros((T + 1, L), dtype=np.uint64), "uniq": np.zeros((T, L), dtype=np.uint64), "tops": np.zeros(T + 1, dtype=np.uint64),
                   "n_units": 0}

    def sweep_state(self):
        out = dict(self.sw, n_leaves=self.n_leaves, thresholds=np.array(self.sweep_list or (), dtype=np.float32))
        out.update(sweep_ref.read_out(self.sw["pass"], self.sw["uniq"], self.sw["tops"]))
        return out

    # ---- settings
    def set_sweep(self, thresholds):
        self.sweep_list = tuple(thresholds) if thresholds else None
        self.sweep_reset()

    def set_taxonomy(self, tax):
        self.tax = tax
        self.nodes = tax_ref.Nodes(self.names(), *tax)
        self.tax_here = np.zeros(self.nodes.n, dtype=np.uint64)
        self.tax_any = np.zeros(self.nodes.n, dtype=np.uint64)

    def tax_below(self):
        below = self.tax_here.copy()
        for v in range(self.nodes.n - 1, 0, -1):
            below[self.nodes.par[v]] += below[v]
        return below

    def clade_below(self):
        below = self.clade_here.copy()
        for c in range(len(below) - 1, 0, -1):
            below[self.cm.par[c]] += below[c]
        return below

    # ---- topology
    def insert(self, genome, name):
        orc.greedy_insert(self.ot, genome, name)
        orc.renumber_preorder(self.ot)
        self.new_leaves()

    def prune(self, depth):
        self.ot.prune(depth)
        self.new_leaves()

    # ---- blocks
    def parse(self, data, fastq, limit):
        seqs, begins, consumed, stop = text_ref.scan(data, fastq, limit, True)
        recs = format_ref.records(data, fastq, limit, True)
        assert [r[1] for r in recs] == seqs
        self.text = dict(stale=False, recs=recs, reads=seqs, fastq=fastq, consumed=consumed, n_bases=sum(map(len, seqs)))
        self.fmt_valid = False
        return self.text

    def prepare(self, reads, quals, paired, params):
        ad, ov, co = self.adapters, self.overlap, self.correct
        cor = None
        if paired and ov and co:
            want = correct_ref.prep_block(reads, quals, ov[0], ov[1], co[0], co[1], *(ad or ((), (), 5, 10)), **params)
            ad_want, cor = want["adapters"], want["corrections"]
            self.note("base corrected in mate 1", cor["n_bases"][0] > 0)
            self.note("base corrected in mate 2", cor["n_bases"][1] > 0)
            self.note("unresolved pair", cor["n_unresolved"] > 0)
            self.note("fragment without qualities", cor["n_no_quality"] > 0)
        if paired and ov:
            want = want if co else overlap_ref.prep_block(reads, quals, ov[0], ov[1], *(ad or ((), (), 5, 10)), **params)
            ad_want = want["adapters"]
            self.note("insert found", want["n_overlapped"] > 0)
            self.note("fragment skipped above 512 bases", want["n_skipped"] > 0)
        elif ad:
            want = ad_want = adapter_ref.prep_block(reads, quals, *ad, paired=paired, **params)
        else:
            want, ad_want = prep_ref.prep_block(reads, quals, paired=paired, **params), None
        self.note("adapter found", ad_want is not None and ad_want["n_found"] > 0)
        self.note("read trimmed", want["n_trimmed"] > 0)
        self.note("read dropped", want["n_kept"] < want["n_reads"])
        self.note("read kept whole", any(want["len"][i] == len(reads[i]) > 0 for i in want["kept"]))
        self.prep = dict(stale=False, want=want, paired=paired, reads=want["kept_reads"], adapters=ad_want, overlap=want if paired and ov else None,
                         corrections=cor, kept=list(want["kept"]), reason=list(want["reason"]), last_deplete=None)
        return self.prep

    def deplete(self, screen, thr, pair_mode):
        """pfq_prep_deplete of the block prepared last against the TreeModel `screen` (pair_mode None, "either" or "both"): the
        reference's result.  The block becomes the survivors; the screen's leaf totals grow and what its last query call left ends,
        as after any query call on it; nothing else of this model changes.  A block without units is a no-op (pfq.h) on both."""
        p = self.prep
        ref = deplete_ref.deplete(p["reads"], screen.ot, thr, paired=pair_mode is not None, both=pair_mode == "both", kept=p["kept"], reason=p["reason"])
        hits_main = oracle_sets(self.ot, ref["survivors"], 1.0) if ref["survivors"] else []
        self.note("unit removed", ref["units_removed"] > 0)
        self.note("survivor that hits the main tree", any(hits_main))
        self.note("read under the screen's k removed", any(len(r) < screen.ot.kmer_size and ref["removed"][i // (2 if pair_mode else 1)]
                                                          for i, r in enumerate(p["reads"])))
        if pair_mode == "both":
            either = deplete_ref.deplete(p["reads"], screen.ot, thr, paired=True, kept=p["kept"], reason=p["reason"])
            self.note("fragment removed in mode both", ref["units_removed"] > 0)
            self.note("fragment kept in both that either would remove", any(e and not b for e, b in zip(either["removed"], ref["removed"])))
        self.note("corrected block depleted", p["corrections"] is not None and sum(p["corrections"]["n_bases"]) > 0 and ref["n_units"] > 0)
        self.note("screen result invalidated by a depletion", ref["n_units"] > 0 and (screen.fmt_valid or any(v is not None for v in screen.last.values())))
        self.note("depletion while format_text is valid", self.fmt_valid and ref["n_units"] > 0)
        p.update(reads=ref["survivors"], kept=ref["kept"], reason=ref["reason"], last_deplete=(thr, pair_mode))
        if ref["n_units"]:
            names = screen.names()
            for c, n in enumerate(ref["leaf_counts"]):
                screen.total[names[c]] += n
            screen.refused_query()
        return ref

    # ---- query calls
    def refused_query(self):
        """A query call that was refused: like every query call it ends the validity of what the one before it left."""
        self.last = dict(lca=None, taxa=None, best=None, scores=None)
        self.fmt_valid = False

    def classify(self, reads, thr, *, paired=None, hits=False, scores=False, lca=None, taxa=False, abundance=False, coverage=False, best=False,
                 sweep=False, log_fits=True):
        """One query call of `reads` (paired: "either" / "both", reads 2i and 2i + 1 are mates): what it returns and leaves behind,
        and every accumulator grown by it."""
        ot = self.ot
        sets = combine(mate_sets(ot, reads, thr), paired) if paired else oracle_sets(ot, reads, thr)
        names = self.names()
        for s in sets:
            for c in s:
                self.total[names[c]] += 1
        offs, leaves = csr_of(sets)
        exp = dict(sets=sets, offs=offs, leaves=leaves, scores=None, lca=None, taxa=None, best=None, n_units=len(sets))
        self.note("empty row", any(not s for s in sets))
        self.note("non-empty row", any(s for s in sets))
        sc = None
        if scores:
            sc = pair_scores(ot, reads, sets, self.contains) if paired else expected_scores(ot, reads, offs, leaves, self.contains)
            exp["scores"] = np.asarray(sc, dtype=np.int64)
        top = best_sets(sets, sc) if best or lca == "best" else None
        rows = top if best else sets
        if lca:
            exp["lca"] = self.cm.expected(top if lca == "best" else sets)
            self.clade_here += self.cm.here_below(exp["lca"])[0]
        if taxa:
            exp["taxa"], here, _, any_ = self.nodes.counts(rows)
            self.tax_here += here
            self.tax_any += any_
        if abundance and log_fits:
            abund_ref.add(self.log, rows_of(rows))
            self.note("ambiguous abundance row", self.log["n_ambiguous"] > 0)
        if coverage:
            if paired:
                self.sketcher.add_pairs(rows_of(rows), [(reads[2 * f], reads[2 * f + 1]) for f in range(len(sets))])
            else:
                self.sketcher.add_reads(rows_of(rows), reads)
        if best:
            exp["best"] = csr_of(top)
            self.note("best row shorter than its row", any(len(b) < len(s) for b, s in zip(top, sets)))
        if sweep:
            st = sweep_ref.sweep(rows_of(sets), sc, [len(r) for r in reads], K, self.sweep_list, self.n_leaves)
            for k in ("pass", "uniq", "tops"):
                self.sw[k] += st[k]
            self.sw["n_units"] += st["n_units"]
            out = self.sweep_state()
            self.note("sweep counts differ between thresholds", len(self.sweep_list) > 1 and not np.array_equal(out["leaf_units"][0], out["leaf_units"][-1]))
        self.last = {k: exp[k] for k in ("lca", "taxa", "best", "scores")}
        self.fmt_valid = False
        return exp

    def frames(self, seqs, F, S, thr):
        """pfq_query_frames: per sequence its segments' (leaf, first_frame, n_frames, begin, end) from frames_ref.frame_sets, the
        frames in all; the leaf counters grow by one per (sequence, distinct leaf among its segments)."""
        all_sets = frames_ref.frame_sets(self.ot, seqs, F, S, thr)
        names, per_seq = self.names(), []
        for x, sets in zip(seqs, all_sets):
            fr, segs = frames_ref.frame_starts(len(x), F, S), []
            assert len(fr) == len(sets)
            for j0, h in enumerate(sets):
                for l in sorted(h):
                    if j0 and l in sets[j0 - 1]:
                        continue
                    j1 = j0
                    while j1 + 1 < len(sets) and l in sets[j1 + 1]:
                        j1 += 1
                    segs.append((l, j0, j1 - j0 + 1, fr[j0][0], fr[j1][0] + fr[j1][1]))
            per_seq.append(segs)
            for l in {s[0] for s in segs}:
                self.total[names[l]] += 1
        self.note("frames call with a segment", any(per_seq))
        self.note("frames call without a segment", not any(per_seq))
        self.refused_query()            # (a frames call is a query call: it ends the validity of everything the last one left)
        return per_seq, sum(len(s) for s in all_sets)

    def format(self, first, block, pos=True, neg=True):
        """What pfq_text_format must give now (None: PFQ_ERR_STATE) and the whole output in record order."""
        if not self.fmt_valid:
            return None
        recs, rows, names = self.text["recs"], self.fmt_rows, [t.encode() for t in self.names()]
        want = format_ref.format_ref(recs, rows, names, first, block, pos, neg)
        whole = format_ref.dict_all(recs, rows, names, first, block, pos, neg)
        self.note("valid format with both streams", len(want["pos"]) > 0 and len(want["neg"]) > 0)
        self.note("HEAD or TAIL run", any(l[4] in (format_ref.HEAD, format_ref.TAIL) for l in want["left"]))
        self.note("whole block", want["pos_records"] + want["neg_records"] > 0)
        return want, whole


# ---------------------------------------------------------------------------------------------------------------
# the blocks
# ---------------------------------------------------------------------------------------------------------------
class World:
    """The genomes of a tree and the reads drawn from them (tests/test_gpu_parity.RNG, as the workloads of the call sequences)."""

    def __init__(self, genomes, fam, singles, screen=()):
        self.genomes, self.fam, self.singles, self.screen = list(genomes), list(fam), list(singles), list(screen)

    def piece(self, L, of=None):
        of = self.genomes if of is None else of
        g = of[int(RNG.integers(0, len(of)))]
        L = min(L, len(g))
        o = int(RNG.integers(0, len(g) - L + 1))
        return g[o:o + L]

    def screen_piece(self, L):
        """A piece of one of the screen's genomes (of the main tree's where the world has no screen)."""
        return self.piece(L, self.screen or None)

    def screen_reads(self, n):
        """n reads for a query of the screen: of its genomes, of the main tree's, random ones, and the lengths round its k."""
        out = [self.screen_piece(int(RNG.integers(0, 301))) if i % 3 == 0 else self.piece(int(RNG.integers(0, 301))) if i % 3 == 1 else
               rand_dna(int(RNG.integers(0, 301))) for i in range(n)]
        return out + [self.screen_piece(L) for L in (UNDER_K, UNDER_K + 1, UNDER_K + 3, 600)]

    def long_read(self, L):
        out = b""
        while len(out) < L:
            out += self.piece(int(RNG.integers(200, 1500))) + rand_dna(int(RNG.integers(0, 200)))
        return out[:L]

    def varied(self, n, longs=(600, 4097, 9000)):
        """n reads of 0 .. 300 bases, a fifth of them random, and one read of every length of `longs`."""
        out = [self.piece(int(RNG.integers(0, 301))) if i % 5 else rand_dna(int(RNG.integers(0, 301))) for i in range(n)]
        return out + [self.long_read(L) for L in longs]

    def reads(self, rng, small):
        if small:
            kind = ("negative", "single", "family", "short", "errors")[int(rng.integers(0, 5))]
            return workload(kind, self.genomes, self.fam, self.singles, 40)[:40] + self.varied(24, longs=(600,) if rng.random() < 0.7 else (4097,))
        kind = ("negative", "single", "family", "short", "long", "errors")[int(rng.integers(0, 6))]
        n = int(rng.choice([64, 150, 400, 1400]))
        return workload(kind, self.genomes, self.fam, self.singles, n * 3 // 4) + self.varied(n // 4)

    def pairs(self, n, quals=False):
        """n fragments as mates 2i, 2i + 1: inserts of 25 .. 400 bases from the genomes, every fourth from the screen's, read from
        both ends (read-through below the mate length: the adapter follows), unrelated mates, one fragment with a mate above 512
        bases, and the fragments whose fate differs between the pair modes of a depletion: a mate under the screen's k beside a
        screen mate and beside a random one, a screen mate beside a main one.  With `quals` (reads, qualities): a low-quality eighth
        at every 3' end, and in overlaps of 40 pairs or more two planted disagreements (the idea of test_gpu_correct.planted_q) —
        by turns a wrong base of low quality in mate 2 against a high one, the same in mate 1, a wrong base with both qualities
        high (unresolved), an N of low quality in mate 1; every twelfth fragment has a second mate without qualities."""
        out, qs = [], []
        tail = lambda L: bytearray(b"I" * (L - L // 8) + b"#" * (L // 8))
        other = lambda c: b"ACGT"[(b"ACGT".find(bytes([c])) + 1 + int(RNG.integers(0, 3))) % 4]
        for i in range(n):
            L1, L2 = int(RNG.integers(60, 200)), int(RNG.integers(60, 200))
            if i % 4 == 3:
                out += [self.screen_piece(L1) if i % 8 == 7 else self.piece(L1), rand_dna(L2)]
                qs += [bytes(tail(len(out[-2]))), bytes(tail(L2))]
                continue
            ins = self.screen_piece(int(RNG.integers(25, 400))) if i % 4 == 1 else self.piece(int(RNG.integers(25, 400)))
            a, b = bytearray((ins + AD33 + rand_dna(L1))[:L1]), bytearray((orc.revcomp(ins) + AD2 + rand_dna(L2))[:L2])
            q1, q2 = tail(L1), tail(L2)
            I = len(ins)
            lo, hi = max(0, I - L2), min(I, L1)
            if hi - lo >= 40:                        # 2 of 40 or more: inside every tolerance of OVERLAPS
                for t, at in enumerate((lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3)):
                    j, kind = I - 1 - at, (i // 4 + t) % 4
                    if kind == 0:
                        b[j], q1[at], q2[j] = other(b[j]), Q_HIGH, Q_LOW
                    elif kind == 1:
                        a[at], q1[at], q2[j] = other(a[at]), Q_LOW, Q_HIGH
                    elif kind == 2:
                        a[at], q1[at], q2[j] = other(a[at]), Q_HIGH, Q_HIGH
                    else:
                        a[at], q1[at], q2[j] = ord("N"), Q_LOW, Q_HIGH
            out += [bytes(a), bytes(b)]
            qs += [bytes(q1), None if i % 12 == 5 else bytes(q2)]
        more = [self.long_read(600), self.piece(150), b"", self.piece(100), self.piece(UNDER_K), self.screen_piece(100), self.piece(UNDER_K), rand_dna(100),
                self.screen_piece(120), self.piece(120)]
        out += more
        qs += [bytes(tail(len(r))) if len(r) > 2 * UNDER_K else b"I" * len(r) for r in more]
        return (out, qs) if quals else out

    def prep_reads(self, n, with_quals):
        """Reads for the trimmer: plain ones, low-quality and poly-G tails, adapter read-through, random, short, N-rich and
        homopolymer reads, 0 .. 300 bases, every third from the screen's genomes, three long ones that carry an adapter, and two
        of UNDER_K bases: min_length = K keeps them, and the screen, whose k is larger, finds no k-mer in them."""
        reads, quals = [], []
        for i in range(n):
            L = int(RNG.integers(0, 301))
            s, q = bytearray(self.screen_piece(L) if i % 3 == 1 else self.piece(L)), bytearray(b"I" * L)     # (every kind from both trees' genomes)
            kind = i % 8
            if kind == 1 and L > 50:
                t = int(RNG.integers(5, 40))
                q[L - t:] = b"#" * t
            elif kind == 2 and L > 50:
                s[L - 13] = ord("A")
                s[L - 12:] = b"G" * 12
            elif kind == 3 and L > 60:
                p = int(RNG.integers(30, L - 10))
                s[p:] = (AD33 + rand_dna(L))[:L - p]
            elif kind == 4:
                s = bytearray(rand_dna(L))
            elif kind == 5:
                s, q = s[:min(L, int(RNG.integers(0, K)))], q[:min(L, K - 1)]
                q = q[:len(s)]
            elif kind == 6 and L > 20:
                for j in RNG.integers(0, L, 8).tolist():
                    s[j] = ord("N")
            elif kind == 7:
                s = bytearray(b"T" * L)
            reads.append(bytes(s))
            quals.append(bytes(q))
        for L in (600, 4097, 9000):
            x = self.long_read(L)
            p = L - int(RNG.integers(40, 200))
            reads.append((x[:p] + AD33 + rand_dna(L))[:L])
            quals.append(b"I" * (L - 20) + b"#" * 20)
        for x in (self.piece(UNDER_K), self.screen_piece(UNDER_K)):     # kept by min_length = K, under the screen's k
            reads.append(x)
            quals.append(b"I" * len(x))
        return reads, (quals if with_quals else None)

    def sequences(self, F, S, negative):
        """Long sequences for a frames call: chimeras and planted inserts, the lengths where the frame rule changes, unrelated ones."""
        r = rand_dna
        if negative:
            return [r(n) for n in (K, 90, 300, 1500)]                 # (a sequence without k-mers would pass every leaf)
        if (F, S) == (K, 1):
            return [self.piece(n) for n in (0, 4, K - 1, K, K + 1, 64, 130)] + [r(90)]
        g = self.genomes
        return [r(700) + g[-1][200:1200] + r(500), g[0][0:1200] + g[-2][300:1500], r(400) + g[3][100:1300] + r(300), g[-3], r(1500), r(300),
                self.long_read(4097)] + [g[-1][300:300 + n] for n in (0, K - 1, K, F - 1, F, F + 1, F + S + 1)]


def balanced_case():
    """The tree of the `balanced` fixture of tests/test_gpu_call_sequences.py: (genomes, ids, oracle tree, World)."""
    fam = close_families(3)
    singles = [rand_dna(3000) for _ in range(6)]
    ot, ids = oracle_tree(fam + singles, K, 131071, 7)
    return fam + singles, ids, ot, World(fam + singles, fam, singles, screen=[rand_dna(3000) for _ in range(3)])


def balanced_screen(world):
    """The screen that lives beside the balanced tree, over world.screen: (ids, a new oracle tree)."""
    s = SCREEN_BALANCED
    ids = [f"S{i:02d}" for i in range(len(world.screen))]
    return ids, orc.build_balanced_tree(world.screen, ids, s["k"], s["nbits"], s["h"], *s["seeds"])


def greedy_screen(world, seed):
    """The screen beside the greedy tree: (ids, a new greedy oracle tree, the one genome it still takes)."""
    s = SCREEN_GREEDY
    ids = [f"S{seed}_{i}" for i in range(len(world.screen))]
    return ids, orc.build_greedy_tree(world.screen, ids, s["k"], s["fpr"], s["largest"], *s["seeds"]), [(world.screen_spare, f"S{seed}_x")]


def greedy_case(seed):
    """The tree of test_greedy_tree_sequence_with_inserts: (genomes, ids, oracle tree, World, the two genomes it still takes)."""
    base = rand_dna(3000)
    fam = [base] + [mutate(base, 2) for _ in range(5)]
    singles = [rand_dna(int(RNG.integers(2500, 3500))) for _ in range(4)]
    genomes = fam + singles
    ids = [f"M{seed}_{i}" for i in range(len(genomes))]
    ot = orc.build_greedy_tree(genomes, ids, K, 0.001, 5000, 5, 10)
    extra = [(mutate(base, 3), f"M{seed}_x0"), (rand_dna(3000), f"M{seed}_x1")]
    world = World(genomes, fam, singles, screen=[rand_dna(3000) for _ in range(3)])
    world.screen_spare = rand_dna(3000)
    return genomes, ids, ot, world, extra


BALANCED_SEED, GREEDY_SEED = 8100, 8300
# what one sequence's expectations must hold, from the references alone (TreeModel.seen)
NOT_VACUOUS = ("non-empty row", "empty row", "ambiguous abundance row", "read trimmed", "read dropped", "read kept whole", "adapter found", "insert found",
               "fragment skipped above 512 bases", "valid format with both streams", "HEAD or TAIL run", "whole block", "frames call with a segment",
               "frames call without a segment", "sweep counts differ between thresholds", "best row shorter than its row", "paired text query with hits",
               # the depletion and the mate correction
               "unit removed", "survivor that hits the main tree", "fragment removed in mode both", "fragment kept in both that either would remove",
               "read under the screen's k removed", "second call removes nothing", "base corrected in mate 1", "base corrected in mate 2", "unresolved pair",
               "fragment without qualities", "corrected block depleted", "screen result invalidated by a depletion", "depletion while format_text is valid")


# ---------------------------------------------------------------------------------------------------------------
# comparisons of read-outs
# ---------------------------------------------------------------------------------------------------------------
def raises(code, call, *args, **kw):
    try:
        call(*args, **kw)
    except PfqError as e:
        assert e.code == code, (e.code, code, str(e))
        return
    raise AssertionError(f"{getattr(call, '__name__', call)} was not refused with {code}")


def same_abundance(got, want, tag):
    for k in ("n_units", "n_unhit", "n_unique", "n_ambiguous", "n_all_leaves", "n_entries", "iterations", "converged", "last_delta"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    for k in ("unique", "mass"):
        assert got[k].tolist() == [int(x) for x in want[k]], (tag, k)


def same_coverage(got, ref, tag):
    sk = ref.sk
    assert (got["n_leaves"], got["precision"], got["n_units"]) == (sk.n_leaves, sk.p, sk.n_units), (tag, got["n_units"], sk.n_units)
    assert np.array_equal(got["registers"], np.array(sk.registers, dtype=np.uint8)), tag
    for k, want in (("units", sk.units), ("matched", sk.matched), ("filter_bits", ref.filter_bits())):
        assert got[k].tolist() == want, (tag, k, got[k].tolist(), want)
    assert np.allclose(got["distinct"], sk.distinct(), rtol=1e-9, atol=0.0), tag


def check_accumulators(gt, m, tag):
    """Every accumulator of the tree against the model."""
    check_counts(gt, m)
    here, below = gt.clade_counts()
    assert np.array_equal(here, m.clade_here) and np.array_equal(below, m.clade_below()), (tag, "clades", here.tolist(), m.clade_here.tolist())
    if m.nodes is None:
        assert gt.taxa() == [], tag
    else:
        assert gt.taxa() == m.nodes.table, tag
        t_here, t_below, t_any = gt.taxon_counts()
        assert np.array_equal(t_here, m.tax_here) and np.array_equal(t_below, m.tax_below()) and np.array_equal(t_any, m.tax_any), (tag, "taxa")
    if m.log_ok:
        same_abundance(gt.abundance(200, 0), abund_ref.estimate(m.log, 200, 0), tag)
    else:
        raises(PFQ_ERR_STATE, gt.abundance)
    same_coverage(gt.coverage(), m.sketcher, tag)
    sweep_ref.same(gt.sweep(), m.sweep_state(), tag)


def check_last(gt, m, tag):
    """last_lca / last_taxa / last_best_rows / last_hit_scores: equal to what the last call left while valid, refused otherwise."""
    last = m.last
    if last["lca"] is None:
        raises(PFQ_ERR_ARG, gt.last_lca)
    else:
        assert np.array_equal(gt.last_lca(), last["lca"]), (tag, "last_lca")
    if last["taxa"] is None:
        raises(PFQ_ERR_ARG, gt.last_taxa)
    else:
        assert np.array_equal(gt.last_taxa(), last["taxa"]), (tag, "last_taxa")
    if last["best"] is None:
        raises(PFQ_ERR_ARG, gt.last_best_rows)
    else:
        offs, leaves = gt.last_best_rows()
        assert np.array_equal(offs, last["best"][0]) and np.array_equal(leaves, last["best"][1]), (tag, "last_best_rows")
    if last["scores"] is None:
        raises(PFQ_ERR_ARG, gt.last_hit_scores)
    else:
        assert np.array_equal(np.asarray(gt.last_hit_scores()).astype(np.int64), last["scores"]), (tag, "last_hit_scores")


def check_prep_reports(gt, m, tag):
    """last_adapters / last_overlap / last_corrections of the block prepared last (PFQ_ERR_STATE when that prep did not run the
    step): the totals and, since every prep of a deck asks for the reads, the arrays and the patch list, exact and in order."""
    p = m.prep
    if p is None or p["adapters"] is None:
        raises(PFQ_ERR_STATE, gt.last_adapters)
    else:
        ad = gt.last_adapters()
        for k in ("n_reads", "n_found", "bases_cut", "found"):
            assert ad[k] == p["adapters"][k], (tag, k, ad[k], p["adapters"][k])
        assert np.array_equal(ad["cut"], np.array(p["adapters"]["cut"], dtype=np.uint32)) and ad["which"].tolist() == p["adapters"]["which"], tag
    if p is None or p["overlap"] is None:
        raises(PFQ_ERR_STATE, gt.last_overlap)
    else:
        ov = gt.last_overlap()
        for k in overlap_ref.TOTALS:
            assert ov[k] == p["overlap"][k], (tag, k, ov[k], p["overlap"][k])
        assert ov["hist"].tolist() == p["overlap"]["hist"] and ov["insert"].tolist() == p["overlap"]["insert"], tag
    if p is None or p["corrections"] is None:
        raises(PFQ_ERR_STATE, gt.last_corrections)
    else:
        cor, want = gt.last_corrections(), p["corrections"]
        for k in correct_ref.TOTALS:
            assert cor[k] == want[k], (tag, k, cor[k], want[k])
        got = list(zip(*(cor["patches"][k].tolist() for k in ("read", "pos", "base", "qual", "old_base", "old_qual"))))
        assert got == want["patches"], (tag, "patches", got[:4], want["patches"][:4])     # (every prep of a deck asks for the reads)


def check_prep_csr(gt, reads, tag):
    """The prepared CSR on the device, byte for byte, against the reads the model holds."""
    cseq, coff = gt.prep_csr()
    assert coff.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in reads], dtype=np.int64)]).tolist(), (tag, "csr offsets")
    assert cseq.tobytes() == b"".join(reads), (tag, "csr bytes")


def check_format(gt, m, first, block, tag):
    """format_text now: byte for byte the reference's when valid (twice: the same result), else PFQ_ERR_STATE."""
    want = m.format(first, block)
    if want is None:                                    # refused, and nothing is written: the caller's struct is as it was
        out = _ffi.TextRecords(n_records=0x1111, pos_records=0x2222, neg_records=0x3333, pos_bytes=0x4444, neg_bytes=0x5555, n_left=0x6666)
        before = bytes(out)
        rc = _ffi.lib().pfq_text_format(gt._h, first, block, _ffi.FMT_POS | _ffi.FMT_NEG, C.byref(out))
        assert rc == PFQ_ERR_STATE and bytes(out) == before, (tag, rc)
        return None
    want, whole = want
    got = gt.format_text(first, block)
    assert got["left"] == want["left"], (tag, got["left"], want["left"])
    assert (got["n_records"], got["pos_records"], got["neg_records"]) == (want["n_records"], want["pos_records"], want["neg_records"]), tag
    assert got["pos"] == want["pos"] and got["neg"] == want["neg"], tag
    names = [t.encode() for t in m.names()]
    assert format_ref.splice(got, m.text["recs"], m.fmt_rows, names, first, block) == whole, tag
    assert gt.format_text(first, block) == got, tag
    return got


# ---------------------------------------------------------------------------------------------------------------
# one deck on one tree
# ---------------------------------------------------------------------------------------------------------------
class Side:
    """One of the two trees of a Play: its model and, on a device, the tree and its Runner."""

    def __init__(self, m, gt=None, runner=None, extra=()):
        self.m, self.gt, self.runner = m, gt, runner
        self.extra = list(extra)        # genomes a greedy tree still takes: (genome, name)


class Play:
    """Runs a deck on a TreeModel and, with `gt` and `runner` (the Runner of tests/test_gpu_call_sequences.py), on the tree itself,
    every call checked as it returns; `screen` is the Side of the second tree, the one prepared blocks are depleted against, which
    lives beside the first for the whole deck.  Everything is drawn from `rng` on the model's side, so a deck runs the same way
    with and without a device."""

    def __init__(self, model, world, seed, gt=None, runner=None, extra=(), screen=None):
        self.m, self.w, self.rng, self.gt, self.runner = model, world, np.random.default_rng(seed), gt, runner
        self.main = Side(model, gt, runner, extra)
        self.extra = self.main.extra
        self.screen = screen
        self.n_frames = self.n_unsynced = self.most_unsynced = 0
        self.step = 0
        self.read_steps = set()         # the steps whose query call was followed by a read of its results or of the counters

    # ---- drawing
    def threshold(self, sweep_wanted, m=None):
        m = m or self.m
        thr = THRESHOLDS[int(self.rng.integers(0, 4))]
        if sweep_wanted and m.sweep_list:
            low = [t for t in THRESHOLDS if np.float32(t) <= np.float32(m.sweep_list[0])]
            thr = low[int(self.rng.integers(0, len(low)))]
        return thr

    def flags(self, mode, n_units, thr, paired, m=None):
        """The flags of a query call: the result mode and independently any legal subset of the post-stages."""
        rng, m = self.rng, m or self.m
        small, forced = n_units <= SMALL, mode
        if mode is None:
            mode = ("counts", "counts", "hits", "scores")[int(rng.integers(0, 4))]
        if mode == "scores" and not small:
            mode = "hits"
        f = dict(hits=mode != "counts", scores=mode == "scores", lca=None, taxa=False, abundance=False, coverage=False, best=False, sweep=False)
        draw = rng.random(6)
        if draw[0] < 0.5:
            f["lca"] = "best" if f["scores"] and draw[0] < 0.25 else "all"
        if f["hits"]:
            f["taxa"] = m.nodes is not None and draw[1] < 0.6
            f["abundance"] = m.log_ok and draw[2] < 0.5
            f["coverage"] = small and draw[3] < 0.5
        if f["scores"]:
            f["best"] = forced == "scores" or draw[4] < 0.5
            f["sweep"] = bool(not paired and m.sweep_list and np.float32(thr) <= np.float32(m.sweep_list[0]) and (forced == "scores" or draw[5] < 0.8))
        return f

    # ---- the device side of a query call
    def query(self, entry, reads, thr, f, paired, side=None):
        side = side or self.main
        gt, runner = side.gt, side.runner
        kw = dict(paired=paired is not None, pair_mode=paired or "either")
        post = {k: f[k] for k in ("lca", "abundance", "coverage", "taxa", "best", "sweep")}
        runner.last_stream = 0
        if entry == "text":
            return gt.query_text(thr, want_hits=f["hits"], want_scores=f["scores"], **kw, **post)
        if entry == "prepq":
            return gt.query_prep(thr, want_hits=f["hits"], want_scores=f["scores"], **kw, **post)
        seq, off = pack_reads(reads)
        if entry == "host":
            return gt.query_packed(seq, off, thr, want_hits=f["hits"], want_scores=f["scores"], **kw, **post)
        stream = 0
        if entry == "streams":
            runner.which ^= 1
            stream = runner.last_stream = runner.streams[runner.which]
        d_seq, d_off, total = runner.device(seq, off, entry)
        if f["hits"]:
            res = gt.query_device_hits(d_seq, d_off, len(reads), total, thr, stream=stream, want_scores=f["scores"], **kw, **post)
            return tuple(np.array(x) for x in res)
        gt.query_device(d_seq, d_off, len(reads), total, thr, stream=stream, lca=f["lca"], **kw)
        return None

    def classify(self, entry, reads, mode, paired=None, thr=None, side=None):
        """One query call through `entry`: the model's expectation, the call, and the checks that belong to it."""
        side = side or self.main
        m, gt, rng = side.m, side.gt, self.rng
        n_units = len(reads) // 2 if paired else len(reads)
        if thr is None:
            thr = self.threshold(not paired and n_units <= SMALL and mode in (None, "scores"), m)
        f = self.flags(mode, n_units, thr, paired, m)
        exp = m.classify(reads, thr, paired=paired, **f)
        tag = (self.step, entry, thr, paired, {k: v for k, v in f.items() if v}) + (("screen",) if side is self.screen else ())
        read_now = f["hits"] or (rng.random() < 0.25 and mode != "counts")     # (a forced counts-only call is never read: PAIRS)
        if read_now:
            self.read_steps.add(self.step)
        if gt is not None:
            gt.set_path(int(rng.choice([-1, 1])))
            res = self.query(entry, reads, thr, f, paired, side)
            if f["hits"]:
                assert np.array_equal(res[0], exp["offs"]) and np.array_equal(res[1], exp["leaves"]), tag
                if f["scores"]:
                    assert np.array_equal(np.asarray(res[2]).astype(np.int64), exp["scores"]), tag
            else:
                assert res is None, tag
            if read_now:
                check_last(gt, m, tag)
                check_counts(gt, m)
        else:
            rng.choice([-1, 1])
        if read_now:                                    # (most counts-only calls are followed by another call unsynchronised)
            self.n_unsynced = 0
        else:
            self.n_unsynced += 1
            self.most_unsynced = max(self.most_unsynced, self.n_unsynced)
        return exp, f

    # ---- query operations
    def op_host(self, mode):
        small = mode == "scores" or (mode is None and self.rng.random() < 0.4)
        paired = (None, None, "either", "both")[int(self.rng.integers(0, 4))] if mode != "scores" else None
        reads = self.w.pairs(30 if small else 150) if paired else self.w.reads(self.rng, small)
        self.classify("host", reads, mode, paired)

    def op_dev(self, mode):
        small = mode == "scores" or (mode is None and self.rng.random() < 0.4)
        paired = (None, None, None, "either", "both")[int(self.rng.integers(0, 5))]
        reads = self.w.pairs(30 if small else 150) if paired else self.w.reads(self.rng, small)
        entry = ("dev0", "streams", "streams", "bytes0", "window")[int(self.rng.integers(0, 5))]
        self.classify(entry, reads, mode, paired)

    def op_parse(self, mode):
        """FASTQ or FASTA, LF or CRLF, the last line terminated or not, a limit that takes a prefix, PFQ_TEXT_TILE 256 or default."""
        rng = self.rng
        small = rng.random() < 0.5
        reads = self.w.reads(rng, True) if small else self.w.varied(int(rng.choice([64, 150, 250])), longs=(600, 4097))
        fastq, eol, final_newline = bool(rng.integers(0, 2)), (b"\n", b"\r\n")[int(rng.integers(0, 2))], bool(rng.integers(0, 2))
        if mode == "even":
            reads = reads[:len(reads) - len(reads) % 2]
        data = (fc.fastq if fastq else fc.fasta)(reads, eol, final_newline)
        limit = len(data) * 2 // 3 if rng.random() < 0.4 and mode != "even" else None
        tile = "256" if rng.random() < 0.5 else None
        text = self.m.parse(data, fastq, limit)
        if self.gt is not None:
            self.gt.set_option("PFQ_TEXT_TILE", tile)
            try:
                got = self.gt.parse_text(data, "fastq" if fastq else "fasta", limit=limit)
            finally:
                self.gt.set_option("PFQ_TEXT_TILE", None)
            assert (got["n_records"], got["consumed"], got["n_bases"]) == (len(text["recs"]), text["consumed"], text["n_bases"]), (self.step, got)

    def op_text(self, mode):
        if self.m.text is None:
            self.op_parse(None)
        m = self.m
        reads = m.text["reads"]
        paired = "either" if mode is None and len(reads) % 2 == 0 and self.rng.random() < 0.15 else None
        if mode == "paired":            # the block of a ("parse", "even") before it, as fragments
            assert len(reads) % 2 == 0 and len(reads) > 0
            paired, mode = ("either", "both")[int(self.rng.integers(0, 2))], "hits"
        m.note("paired text query with hits", paired is not None and mode == "hits")
        thr = (1.0, 0.7, 0.3)[int(self.rng.integers(0, 3))] if mode == "hits" else None   # (at 0 every record is mapped: no NEG stream)
        m.note("parsed block queried after the leaves changed", m.text["stale"])
        exp, f = self.classify("text", reads, mode, paired, thr)
        m.fmt_valid = f["hits"] and not paired          # pfq.h "text output": a successful pfq_text_query with PFQ_WANT_HITS, without PFQ_PAIRED
        m.fmt_rows = rows_of(exp["sets"])

    def prepare(self, paired, mode=None):
        rng, m = self.rng, self.m
        params = PREP_PARAMS[int(rng.integers(0, len(PREP_PARAMS)))]
        with_quals = rng.random() < 0.7 or mode == "quals"
        if paired:
            reads, quals = self.w.pairs(int(rng.choice([20, 34])), quals=True)
            quals = quals if with_quals else None
        else:
            reads, quals = self.w.prep_reads(int(rng.choice([64, 200, 600])), with_quals)
        p = m.prepare(reads, quals, paired, params)
        if self.gt is not None:
            if quals is None:
                (seq, off), qual, hq = pack_reads(reads), None, None
            else:
                seq, off, qual, hq = pack_quals(reads, quals)
            got = self.gt.prep_reads(seq, off, qual, hq, paired=paired, want_reads=True, **params)
            want = p["want"]
            for k in ("n_reads", "n_kept", "bases_in", "bases_kept", "n_trimmed", "n_reason"):
                assert got[k] == want[k], (self.step, k, got[k], want[k])
            for k in ("begin", "len", "reason", "kept"):
                assert np.array_equal(got[k], np.array(want[k], dtype=np.uint32)), (self.step, k)
            check_prep_csr(self.gt, p["reads"], (self.step, "prep"))
            check_prep_reports(self.gt, m, (self.step, "prep"))

    def op_prep(self, mode):
        self.prepare(False)

    def op_prep_paired(self, mode):
        self.prepare(True, mode)

    def op_prepq(self, mode):
        m = self.m
        if m.prep is None:
            self.prepare(False)
        paired = (("either", "both")[int(self.rng.integers(0, 2))]) if self.whole_fragments() else None
        m.note("prepared block queried after the leaves changed", m.prep["stale"])
        self.classify("prepq", m.prep["reads"], mode, paired)

    def whole_fragments(self):
        """Whether the block prepared last still consists of fragments: prepared paired and never depleted read by read."""
        return self.m.prep["paired"] and not self.m.prep.get("split")

    # ---- the second tree
    def op_deplete(self, mode):
        """pfq_prep_deplete of the block prepared last against the screen ("again": the call before it repeated, which removes
        nothing), and after it everything the call may and may not have touched, on both trees."""
        m, rng, scr = self.m, self.rng, self.screen
        if m.prep is None:
            self.prepare(False)
        p = m.prep
        if mode == "again" and p["last_deplete"] is not None:
            thr, pair_mode = p["last_deplete"]
        else:
            thr = THRESHOLDS[int(rng.integers(0, 4 if mode is None else 3))]
            pair_mode = (None, "either", "both")[int(rng.integers(0, 3))] if self.whole_fragments() else None
            if mode in ("either", "both") and self.whole_fragments():
                pair_mode = mode
        before = dict(m.last), m.fmt_valid, dict(m.total)
        ref = m.deplete(scr.m, thr, pair_mode)
        if mode == "again":
            assert ref["units_removed"] == 0 and ref["n_units"] * (2 if pair_mode else 1) == ref["n_kept"], (self.step, ref["units_removed"])
            m.note("second call removes nothing", ref["n_units"] > 0)
        if p["paired"] and pair_mode is None and ref["units_removed"]:
            p["split"] = True                        # (mates were judged one by one: the survivors are reads)
        assert all(m.last[k] is before[0][k] for k in m.last) and m.fmt_valid == before[1] and m.total == before[2]
        self.n_unsynced = 0
        if self.gt is None:
            return
        tag = (self.step, "deplete", thr, pair_mode)
        got = self.gt.prep_deplete(scr.gt, thr, paired=pair_mode is not None, pair_mode=pair_mode or "either")
        for k in deplete_ref.TOTALS:
            assert got[k] == ref[k], (tag, k, got[k], ref[k])
        for k in ("kept", "reason"):
            assert np.array_equal(got[k], np.array(ref[k], dtype=np.uint32)), (tag, k)
        check_prep_csr(self.gt, ref["survivors"], tag)
        check_prep_reports(self.gt, m, tag)
        self.check_both(tag)

    def op_screen_query(self, mode):
        """A query of the screen, so that a depletion has something to invalidate: through the host or a device stream; "text": its
        own parse_text, query_text with hits and format_text."""
        scr, rng = self.screen, self.rng
        reads = self.w.screen_reads(40)
        if mode == "text":
            data = fc.fastq(reads)
            text = scr.m.parse(data, True, None)
            if scr.gt is not None:
                got = scr.gt.parse_text(data, "fastq")
                assert (got["n_records"], got["consumed"], got["n_bases"]) == (len(text["recs"]), text["consumed"], text["n_bases"]), (self.step, got)
            exp, f = self.classify("text", text["reads"], "hits", None, 0.7, side=scr)
            scr.m.fmt_valid, scr.m.fmt_rows = True, rows_of(exp["sets"])
            if scr.gt is not None:
                assert check_format(scr.gt, scr.m, 0, 7, (self.step, "screen format")) is not None
            return
        paired = (None, None, "either", "both")[int(rng.integers(0, 4))]
        reads = reads[:len(reads) - len(reads) % 2]
        entry = ("host", "streams", "dev0")[int(rng.integers(0, 3))]
        self.classify(entry, reads, mode, paired, side=scr)

    def op_screen_insert(self, mode):
        scr = self.screen
        genome, name = scr.extra.pop(0)
        if scr.gt is not None:
            scr.runner.sync()
            scr.gt.insert(genome, name)
        scr.m.insert(genome, name)
        self.w.screen.append(genome)

    def frames(self, device):
        m, rng = self.m, self.rng
        F, S = GRID[int(rng.integers(0, len(GRID)))]
        negative = self.n_frames % 2 == 1
        self.n_frames += 1
        thr = 1.0 if negative else (1.0, 0.7, 0.3)[int(rng.integers(0, 3))]
        seqs = self.w.sequences(F, S, negative)
        per_seq, n_frames = m.frames(seqs, F, S, thr)
        if self.gt is None:
            return
        seq, off = pack_reads(seqs)
        self.runner.last_stream = 0
        if device:
            d_seq, d_off, total = self.runner.device(seq, off, "dev0")
            offs, segs = self.gt.query_frames_device(d_seq, d_off, len(seqs), total, F, S, thr)
        else:
            offs, segs = self.gt.query_frames(seq, off, F, S, thr)
        tag = (self.step, "frames", F, S, thr)
        assert len(offs) == len(seqs) + 1 and self.gt.last_n_frames == n_frames, tag
        for i, want in enumerate(per_seq):
            got = [tuple(int(s[k]) for k in ("leaf", "first_frame", "n_frames", "begin", "end")) for s in segs[int(offs[i]):int(offs[i + 1])]]
            assert got == want, (tag, i, got, want)
        check_counts(self.gt, m)
        check_last(self.gt, m, tag)

    def op_frames(self, mode):
        self.frames(False)

    def op_frames_dev(self, mode):
        self.frames(True)

    # ---- operations that change nothing
    def op_format(self, mode):
        block = fc.BLOCKS[int(self.rng.integers(0, len(fc.BLOCKS) - 1))]
        first = fc.first_indices(block)[int(self.rng.integers(0, 4)) % len(fc.first_indices(block))]
        if self.gt is not None:
            check_format(self.gt, self.m, first, block, (self.step, "format", first, block))
        else:
            self.m.format(first, block)

    def op_readout(self, mode):
        self.n_unsynced = 0
        if self.gt is None:
            return
        for side in (self.main, self.screen):
            if side is None:
                continue
            gt, m, tag = side.gt, side.m, (self.step, "readout", "screen" if side is self.screen else "main")
            side.runner.sync()
            check_accumulators(gt, m, tag)
            check_last(gt, m, tag)
            check_prep_reports(gt, m, tag)
            info = gt.info()
            assert (int(info.n_leaves), int(info.kmer_size)) == (m.n_leaves, m.ot.kmer_size), tag
            gt.last_stats()
            assert gt.clades() == m.cm.table, tag

    def op_similarity(self, mode):
        if self.gt is not None:
            sim_ref.same(self.gt.similarity(), sim_ref.similarity(self.m.ot), (self.step, "similarity"))

    def op_recluster(self, mode):
        if self.gt is not None:
            log, rounds = cluster_ref.log_of(self.m.ot)
            new = self.gt.recluster()
            try:
                cluster_ref.same_log(new.merges(), log, rounds, new.merge_rounds(), (self.step, "recluster"))
            finally:
                new.close()

    def op_option(self, mode):
        """A result-neutral knob set to a value and back; a format_text that was valid is still valid and byte-exact under it."""
        name, value = KNOBS[int(self.rng.integers(0, len(KNOBS)))]
        under = {"PFQ_FRAME_PIECE": self.op_frames, "PFQ_SIM_SLICES": self.op_similarity, "PFQ_FMT_GRID": None, "PFQ_FMT_HASH_BITS": None}
        if self.gt is not None:
            self.gt.set_option(name, value)
        try:
            if self.gt is not None:
                check_format(self.gt, self.m, 0, 7, (self.step, "option", name, value))
            else:
                self.m.format(0, 7)
            call = under.get(name, self.op_host)            # the stage the knob steers runs while it is set, checked like any call
            if call is not None:
                call("scores" if name == "PFQ_SWEEP_LDS" else None)
        finally:
            if self.gt is not None:
                self.gt.set_option(name, None)

    def op_delta(self, mode):
        if self.gt is not None:
            self.runner.delta_round_trip(self.m)
        self.n_unsynced = 0

    # ---- operations that change state by the header's rules
    def op_reset_counts(self, mode):
        if self.gt is not None:
            self.runner.sync()
            self.gt.reset_counts()
        self.m.reset()

    def op_abundance_reset(self, mode):
        if self.gt is not None:
            self.gt.abundance_reset()
        self.m.abundance_reset()

    def op_coverage_reset(self, mode):
        if self.gt is not None:
            self.gt.coverage_reset()
        self.m.coverage_reset()

    def op_sweep_reset(self, mode):
        if self.gt is not None:
            self.gt.sweep_reset()
        self.m.sweep_reset()

    def op_set_sweep(self, mode):
        choice = [l for l in SWEEP_LISTS if l != self.m.sweep_list and (l or mode != "on")]
        thresholds = choice[int(self.rng.integers(0, len(choice)))]
        if self.gt is not None:
            self.gt.set_sweep(thresholds or [])
        self.m.set_sweep(thresholds)

    def op_set_taxonomy(self, mode):
        tax = random_taxonomy(int(self.rng.integers(0, 1 << 30)), self.m.n_leaves)
        if self.gt is not None:
            self.gt.set_taxonomy(*tax)
        self.m.set_taxonomy(tax)

    def op_set_adapters(self, mode):
        choice = [a for a in ADAPTER_SETS if a != self.m.adapters and (a or mode != "on")]
        ad = choice[int(self.rng.integers(0, len(choice)))]
        if self.gt is not None:
            if ad is None:
                self.gt.set_adapters([])
            else:
                self.gt.set_adapters(list(ad[0]), list(ad[1]), min_overlap=ad[2], max_error_percent=ad[3])
        self.m.adapters = ad

    def op_set_mate_overlap(self, mode):
        choice = [o for o in OVERLAPS if o != self.m.overlap and (o or mode != "on")]
        ov = choice[int(self.rng.integers(0, len(choice)))]
        if self.gt is not None:
            self.gt.set_mate_overlap(*(ov or (0, 10)))
        self.m.overlap = ov

    def op_set_mate_correct(self, mode):
        choice = [c for c in CORRECTS if c != self.m.correct and (c or mode != "on")]
        co = choice[int(self.rng.integers(0, len(choice)))]
        if self.gt is not None:
            self.gt.set_mate_correct(*(co or (0, 0)))
        self.m.correct = co

    def op_insert(self, mode):
        genome, name = self.extra.pop(0)
        if self.gt is not None:
            self.runner.sync()
            self.gt.insert(genome, name)
        self.m.insert(genome, name)
        self.w.genomes.append(genome)

    def op_prune(self, mode):
        depth = 2 if mode == "deeper" else 3
        if self.gt is not None:
            self.runner.sync()
            self.gt.prune_tree(depth)
        self.m.prune(depth)

    # ---- refused calls
    def refusals(self):
        """[(name, documented code, the call on a tree)] of the refusals that apply to the tree as it is.  Every one is a query call
        refused on the host: like any query call it ends the validity of what the call before it left (pfq.h)."""
        m = self.m
        reads = self.w.reads(self.rng, True)
        seq, off = pack_reads(reads)
        pseq, poff = pack_reads(self.w.pairs(10))
        out = []
        if m.nodes is None:
            out.append(("taxa without a taxonomy", PFQ_ERR_STATE, lambda gt: gt.query_packed(seq, off, 0.7, want_hits=True, taxa=True)))
        if m.sweep_list is None:
            out.append(("sweep without a list", PFQ_ERR_STATE, lambda gt: gt.query_packed(seq, off, 0.0, want_hits=True, want_scores=True, sweep=True)))
        else:
            if m.sweep_list[0] < 1.0:
                out.append(("sweep above the list's lowest", PFQ_ERR_ARG, lambda gt: gt.query_packed(seq, off, 1.0, want_hits=True, want_scores=True, sweep=True)))
            out.append(("sweep of fragments", PFQ_ERR_ARG,
                        lambda gt: gt.query_packed(pseq, poff, 0.0, want_hits=True, want_scores=True, sweep=True, paired=True)))
        if m.prep is not None and not m.prep["paired"]:
            out.append(("paired query of an unpaired block", PFQ_ERR_ARG, lambda gt: gt.query_prep(0.7, want_hits=True, paired=True)))

        def scores_alone(gt):
            hits = _ffi.Hits()
            _ffi.check(_ffi.lib().pfq_query_batch(gt._h, seq.ctypes.data, off.ctypes.data, len(off) - 1, 0.7, _ffi.WANT_SCORES, C.byref(hits)))
        out.append(("scores without hits", PFQ_ERR_ARG, scores_alone))
        return out

    def deplete_refusals(self):
        """[(name, documented code, the call on (tree, screen))] of the refused depletions that apply now.  They are a kind of their
        own: a refused pfq_prep_deplete is no query call on either tree and changes nothing on either (pfq.h "depletion")."""
        out = []
        if self.m.prep is None:
            out.append(("depletion before any prep", PFQ_ERR_STATE, lambda gt, sgt: gt.prep_deplete(sgt, 0.7)))
        elif not self.m.prep["paired"]:
            out.append(("paired depletion of an unpaired block", PFQ_ERR_ARG, lambda gt, sgt: gt.prep_deplete(sgt, 0.7, paired=True)))
        out.append(("the screen is the tree itself", PFQ_ERR_ARG, lambda gt, sgt: gt.prep_deplete(gt, 0.7)))

        def other_flag(gt, sgt):
            res = _ffi.PrepDepleted()
            _ffi.check(_ffi.lib().pfq_prep_deplete(gt._h, sgt._h, 0.7, _ffi.WANT_HITS, C.byref(res)))
        out.append(("a depletion flag other than the three allowed", PFQ_ERR_ARG, other_flag))
        return out

    def check_both(self, tag):
        """Every accumulator, what the last call left and format_text, on both trees against their models."""
        for side in (self.main, self.screen):
            side.runner.sync()
            check_accumulators(side.gt, side.m, tag)
            check_last(side.gt, side.m, tag)
            check_format(side.gt, side.m, 0, 7, tag)

    def op_refuse(self, mode):
        cases = [("query",) + c for c in self.refusals()] + [("deplete",) + c for c in self.deplete_refusals()]
        kind, name, code, call = cases[int(self.rng.integers(0, len(cases)))]
        if kind == "query":
            self.m.refused_query()
        if self.gt is not None:
            self.runner.last_stream = 0
            if kind == "query":
                raises(code, call, self.gt)
            else:
                raises(code, call, self.gt, self.screen.gt)
                check_prep_reports(self.gt, self.m, (self.step, "refused", name))
            self.check_both((self.step, "refused", name))
        self.n_unsynced = 0

    # ---- the deck
    def run(self, d):
        for self.step, (op, mode) in enumerate(d):
            getattr(self, "op_" + op)(mode)
        self.op_readout(None)
