// hsw_gadget_layout.cpp -- the layout walk and the queries on its result (see hsw_gadget_layout.hpp)
#include "hsw_gadget_layout.hpp"

#include <algorithm>

namespace hsw {

void ColumnWalk::calls(const uint8_t *lens, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const uint8_t len = lens[i];
        if (row + len >= rows) {                          // halo2-lib v0.2.x assign_region: next column (A3-iii)
            bc.push_back(cell); bg.push_back((pitch ? pitch : rows) - row);
            row = 0; col++;
        }
        row += len; cell += len;
    }
}

void ColumnWalk::block(const std::vector<uint8_t> &tape, uint64_t G) {
    if (row + G < rows) { row += G; cell += G; }
    else calls(tape.data(), tape.size());
}

int layout_walk(const hsw_shape &shape, const size_t *sizes, size_t n, bool rc_inputs, uint64_t rows,
                const std::vector<DigestOrigin> *decl, Layout *out) {
    size_t m = 0;
    if (hsw_gate_tape(&shape, nullptr, 0, &m) != HSW_OK) return HSW_ERR_INVALID_ARG;
    std::vector<uint8_t> block_tape(m), t;
    hsw_gate_tape(&shape, block_tape.data(), m, nullptr);
    std::vector<uint64_t> bc, bg;
    out->digest_cell0.clear(); out->digest_entry0.clear(); out->digest_lookup0.clear();
    const uint64_t pitch = out->pitch ? out->pitch : rows;
    ColumnWalk w{rows, 0, out->origin_row, 0, bc, bg, pitch};   // the Context's next free row (hsw_gadget_set_origin)
    uint64_t lk = out->origin_lookups, own = 0;
    bool zero = out->origin_zero_loaded;                  // a Context that already caches its zero cell assigns none
    for (size_t h = 0; h < n; h++) {
        if (decl && h < decl->size() && (*decl)[h].set) { // the caller's interlude ends at (column, row)
            const DigestOrigin &d = (*decl)[h];
            if (d.column < out->origin_column || d.row >= rows) return HSW_ERR_INVALID_ARG;
            // (in image cells: a gap that spans columns takes the cells between them along)
            const uint64_t want = (d.column - out->origin_column) * pitch + d.row, here = w.col * pitch + w.row;
            if (want < here || d.lookups < lk) return HSW_ERR_INVALID_ARG;
            if (want > here) { bc.push_back(w.cell); bg.push_back(want - here); }
            w.col = d.column - out->origin_column; w.row = d.row; lk = d.lookups;
        }
        out->digest_lookup0.push_back(lk);
        out->digest_cell0.push_back(w.cell);
        out->digest_entry0.push_back(own);
        hsw_frame_shape fs;
        int rc = hsw_frame_query(&shape, sizes[h], rc_inputs ? 1 : 0, &fs);
        if (rc != HSW_OK) return rc;
        lk += fs.digest_lookups;
        own += fs.digest_lookups;
        for (int section = 0; section < 2; section++) {
            if (section == 1) {
                const uint8_t one = 1;
                if (!zero) { w.calls(&one, 1); zero = true; }   // Context.zero_cell, first load_zero
                for (size_t k = 0; k < sizes[h] / 64; k++) w.block(block_tape, shape.gate_cells_per_block);
            }
            rc = hsw_frame_tape(&shape, sizes[h], rc_inputs ? 1 : 0, section, nullptr, 0, &m);
            if (rc != HSW_OK) return rc;
            t.resize(m);
            hsw_frame_tape(&shape, sizes[h], rc_inputs ? 1 : 0, section, t.data(), m, nullptr);
            w.calls(t.data(), m);
        }
    }
    out->max_rows = rows;
    out->columns = w.col + 1;
    out->lookups_end = lk;
    out->set_breaks(bc, bg);
    return HSW_OK;
}

void Layout::set_breaks(std::vector<uint64_t> &bc, std::vector<uint64_t> &bg) {
    break_cell.swap(bc);
    break_gap.swap(bg);
    break_cum.resize(break_gap.size());
    uint64_t sum = 0;
    for (size_t k = 0; k < break_gap.size(); k++) break_cum[k] = sum += break_gap[k];
}

uint64_t Layout::gap_at(uint64_t cell) const {           // breaks are ascending: a binary search
    const size_t k = (size_t)(std::upper_bound(break_cell.begin(), break_cell.end(), cell) - break_cell.begin());
    return k ? break_cum[k - 1] : 0;
}

void Layout::position(uint64_t cell, uint64_t *column, uint64_t *row) const {
    if (period) cell %= period;                          // the owning Context's own stream cell
    const uint64_t at = cell + origin_row + gap_at(cell);
    if (max_rows) { if (column) *column = origin_column + at / column_pitch(); if (row) *row = at % column_pitch(); }
    else { if (column) *column = origin_column; if (row) *row = at; }
}

uint64_t Layout::image_cell(uint64_t cell) const {
    uint64_t base = 0;
    if (period) {
        const uint64_t h = cell / period;
        base = h * image_cells();
        cell -= h * period;
    }
    return base + cell + (max_rows ? origin_row : 0) + gap_at(cell);
}

uint64_t Layout::lookup_cell(uint64_t entry) const {
    if (digest_entry0.empty()) return origin_lookups + entry;
    const size_t h = (size_t)(std::upper_bound(digest_entry0.begin(), digest_entry0.end(), entry) - digest_entry0.begin()) - 1;
    return digest_lookup0[h] + (entry - digest_entry0[h]);
}

}  // namespace hsw
