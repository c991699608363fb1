// pfq_taxonomy.h — host side of the taxonomy (pfq.h "taxonomy", DESIGN.md §5 "Taxonomy"): the taxonomy file's grammar and the
// node table derived from (taxon_parent, taxon_names, leaf_taxon).  Plain C++, no device: pfq_host.cpp uses it behind
// pfq_taxonomy_read, pfq_taxonomy_nodes and pfq_tree_set_taxonomy.  Every function returns "" or the error's message.
#pragma once
#include <stdint.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/pfq.h"

namespace pfq_taxonomy {

struct File {
    std::vector<uint32_t> parent;     // [n_taxa], parent[0] = PFQ_NO_CLADE
    std::vector<std::string> names;   // [n_taxa], names[0] = "root"
    std::vector<uint32_t> leaf_taxon; // [n_leaves]
    uint64_t lines_considered = 0, lines_other = 0, leaves_without_line = 0;
};

inline std::string trim_spaces(const std::string &s) {
    size_t b = 0, e = s.size();
    while (b < e && s[b] == ' ') ++b;
    while (e > b && s[e - 1] == ' ') --e;
    return s.substr(b, e - b);
}

// The file grammar.  io: the file could not be read (else the message names a line).
inline std::string read_file(const std::string &path, const std::vector<std::string> &leaf_ids, File &out, bool &io) {
    io = false;
    out = File();
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        io = true;
        return "cannot read " + path + ": " + strerror(errno);
    }
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) {
        io = true;
        return "cannot read " + path;
    }
    std::unordered_map<std::string, std::vector<uint32_t>> leaves_of;  // tax_id -> its leaves
    for (size_t l = 0; l < leaf_ids.size(); ++l) leaves_of[leaf_ids[l]].push_back((uint32_t)l);
    out.parent.push_back(PFQ_NO_CLADE);
    out.names.push_back("root");
    out.leaf_taxon.assign(leaf_ids.size(), 0);
    std::vector<uint8_t> placed(leaf_ids.size(), 0);
    std::map<std::pair<uint32_t, std::string>, uint32_t> child;  // (parent taxon, name) -> taxon: a taxon is its whole path
    uint64_t line_no = 0;
    for (size_t p = 0; p < text.size();) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(p, e - p);
        p = e + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const auto where = [&] { return path + ": line " + std::to_string(line_no) + ": "; };
        const size_t t1 = line.find('\t');
        if (t1 == std::string::npos) return where() + "fewer than two tab-separated fields (genome<TAB>lineage)";
        size_t t2 = line.find('\t', t1 + 1);
        if (t2 == std::string::npos) t2 = line.size();
        const std::string genome = line.substr(0, t1), lineage = trim_spaces(line.substr(t1 + 1, t2 - t1 - 1));
        std::vector<std::string> path_names;
        if (!lineage.empty()) {
            for (size_t q = 0;;) {
                size_t s = lineage.find(';', q);
                if (s == std::string::npos) s = lineage.size();
                path_names.push_back(trim_spaces(lineage.substr(q, s - q)));
                if (path_names.back().empty()) return where() + "empty name in the lineage '" + lineage + "'";
                if (s == lineage.size()) break;
                q = s + 1;
            }
        }
        const auto it = leaves_of.find(genome);
        if (it == leaves_of.end()) {
            ++out.lines_other;
            continue;
        }
        ++out.lines_considered;
        uint32_t cur = 0;
        for (const std::string &name : path_names) {
            const auto key = std::make_pair(cur, name);
            const auto c = child.find(key);
            if (c != child.end()) cur = c->second;
            else {
                const uint32_t idx = (uint32_t)out.parent.size();
                out.parent.push_back(cur);
                out.names.push_back(name);
                child.emplace(key, idx);
                cur = idx;
            }
        }
        for (uint32_t l : it->second) {
            if (placed[l] && out.leaf_taxon[l] != cur) return where() + "genome '" + genome + "' has a different lineage on an earlier line";
            placed[l] = 1;
            out.leaf_taxon[l] = cur;
        }
    }
    for (uint8_t x : placed) out.leaves_without_line += !x;
    return "";
}

struct NodeTable {
    std::vector<pfq_taxon> nodes;     // names point into `names`
    std::vector<std::string> names;
    std::vector<uint32_t> rank, leaf_node;  // [n_leaves]
    std::vector<uint32_t> gap;        // [n_leaves - 1] lowest common node of ranks i and i + 1
    uint32_t top = 0;                 // the deepest node above every leaf
};

// The node table of the model: taxa without a genome below are dropped (the root is kept), every genome is a node under its
// taxon, pre-order = a taxon, its genomes in ascending leaf index, then its other child taxa in ascending input index.
inline std::string build_nodes(uint64_t n_leaves, const char *const *leaf_ids, uint64_t n_taxa, const uint32_t *taxon_parent,
                               const char *const *taxon_names, const uint32_t *leaf_taxon, NodeTable &out) {
    out = NodeTable();
    if (n_taxa < 1 || n_taxa >= PFQ_NO_CLADE || !taxon_parent || !taxon_names || (n_leaves && (!leaf_taxon || !leaf_ids)))
        return "taxonomy: at least one taxon (the root), and no NULL table";
    if (n_leaves + n_taxa >= PFQ_NO_CLADE) return "taxonomy: more than 2^32 - 2 nodes";
    if (taxon_parent[0] != PFQ_NO_CLADE) return "taxonomy: taxon 0 is the root, its parent must be PFQ_NO_CLADE";
    for (uint64_t i = 0; i < n_taxa; ++i) {
        if (i && taxon_parent[i] >= i) return "taxonomy: taxon_parent[" + std::to_string(i) + "] = " + std::to_string(taxon_parent[i]) + " is not below " + std::to_string(i);
        if (!taxon_names[i]) return "taxonomy: taxon " + std::to_string(i) + " has no name";
    }
    for (uint64_t l = 0; l < n_leaves; ++l) {
        if (leaf_taxon[l] >= n_taxa) return "taxonomy: leaf_taxon[" + std::to_string(l) + "] = " + std::to_string(leaf_taxon[l]) + " is no taxon (n_taxa = " + std::to_string(n_taxa) + ")";
        if (!leaf_ids[l]) return "taxonomy: leaf " + std::to_string(l) + " has no name";
    }
    std::vector<uint32_t> below(n_taxa, 0);  // genomes anywhere below
    std::vector<std::vector<uint32_t>> genomes(n_taxa), kids(n_taxa);
    for (uint64_t l = 0; l < n_leaves; ++l) {
        ++below[leaf_taxon[l]];
        genomes[leaf_taxon[l]].push_back((uint32_t)l);
    }
    for (uint64_t i = n_taxa; i-- > 1;) below[taxon_parent[i]] += below[i];
    for (uint64_t i = 1; i < n_taxa; ++i)
        if (below[i]) kids[taxon_parent[i]].push_back((uint32_t)i);
    out.rank.assign(n_leaves, 0);
    out.leaf_node.assign(n_leaves, 0);
    std::vector<uint32_t> node_of(n_taxa, PFQ_NO_CLADE), stack{0};
    uint32_t next_rank = 0;
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        const uint32_t v = (uint32_t)out.nodes.size();
        const uint32_t parent = i ? node_of[taxon_parent[i]] : PFQ_NO_CLADE, depth = i ? out.nodes[parent].depth + 1 : 0;
        node_of[i] = v;
        out.nodes.push_back(pfq_taxon{parent, depth, next_rank, below[i], PFQ_NO_CLADE, nullptr});
        out.names.push_back(taxon_names[i]);
        for (uint32_t l : genomes[i]) {
            out.leaf_node[l] = (uint32_t)out.nodes.size();
            out.rank[l] = next_rank;
            out.nodes.push_back(pfq_taxon{v, depth + 1, next_rank++, 1, l, nullptr});
            out.names.push_back(leaf_ids[l]);
        }
        for (size_t c = kids[i].size(); c-- > 0;) stack.push_back(kids[i][c]);
    }
    for (size_t v = 0; v < out.nodes.size(); ++v) out.nodes[v].name = out.names[v].c_str();
    const size_t nn = out.nodes.size();
    out.top = 0;
    while (n_leaves && out.top + 1 < nn && out.nodes[out.top + 1].n_leaves == n_leaves) ++out.top;
    // gap i: from the genome at rank i + 1 upwards, the first node that begins at or before rank i
    std::vector<uint32_t> by_rank(n_leaves, 0);
    for (uint64_t l = 0; l < n_leaves; ++l) by_rank[out.rank[l]] = out.leaf_node[l];
    out.gap.assign(n_leaves ? n_leaves - 1 : 0, 0);
    for (uint64_t r = 0; r + 1 < n_leaves; ++r) {
        uint32_t t = by_rank[r + 1];
        while (out.nodes[t].first_rank > r) t = out.nodes[t].parent;
        out.gap[r] = t;
    }
    return "";
}

}  // namespace pfq_taxonomy
