// extern "C" face of csrc/eval_plan.h for tests/test_evaluation_diversity_cpu.py (built with g++, called through ctypes).
#include "../recsys2019_deeplearning_evaluation_amd/csrc/eval_plan.h"

using namespace mi355rec::evalplan;

extern "C" {

void ep_constants(int64_t *out) {
    out[0] = DIV_MAX_WIDTH;
    out[1] = DIV_SMALL_WIDTH;
    out[2] = (int64_t)DIV_UPLOAD_CHUNK;
}
int ep_width_ok(int width) { return div_width_ok(width); }
int ep_elem_ok(int elem_bytes) { return div_elem_ok(elem_bytes); }
int ep_threads(int width) { return div_threads(width); }
uint64_t ep_cell_offset(int row_item, int col_item, int n_items) { return div_cell_offset(row_item, col_item, n_items); }
int ep_shell(int i, int j) { return div_shell(i, j); }
int ep_run_count(int len) { return div_run_count(len); }
void ep_run(int w, int *out) {
    const DivRun r = div_run(w);
    out[0] = r.shell; out[1] = r.fixed; out[2] = r.count; out[3] = r.column;
}
uint64_t ep_run_cell(int w, const int *items, int q, int n_items) { return div_run_cell(div_run(w), items, q, n_items); }
int ep_cutoff_length(int cutoff, int len) { return div_cutoff_length(cutoff, len); }
int ep_cutoff_shells(int cutoff, int len) { return div_cutoff_shells(cutoff, len); }
double ep_denominator(int cutoff, int len) { return div_denominator(cutoff, len); }
uint64_t ep_matrix_cells(int n_items) { return div_matrix_cells(n_items); }
uint64_t ep_matrix_bytes(int n_items, int elem_bytes) { return div_matrix_bytes(n_items, elem_bytes); }
uint64_t ep_value_cells(int n_eval, int n_cut) { return div_value_cells(n_eval, n_cut); }
uint64_t ep_upload_chunks(uint64_t bytes) { return div_upload_chunks(bytes); }
int ep_range_blocks(uint64_t cells) { return div_range_blocks(cells); }

// One list the way eval_diversity_kernel walks it: every run summed in ascending order, a cutoff's numerator the running sum of its
// shells (column run + row run), ascending.  out[c] is NaN for a cutoff that sees fewer than two items.
void ep_list_values(const double *D, int n_items, const int *items, int len, const int *cut, int n_cut, double *run_sums, double *out) {
    const int n_runs = div_run_count(len);
    for (int w = 0; w < n_runs; ++w) {
        const DivRun r = div_run(w);
        double s = 0.0;
        for (int q = 0; q < r.count; ++q) s += D[div_run_cell(r, items, q, n_items)];
        run_sums[w] = s;
    }
    for (int c = 0; c < n_cut; ++c) {
        const int shells = div_cutoff_shells(cut[c], len);
        out[c] = __builtin_nan("");
        if (shells > 0) {
            double numerator = 0.0;
            for (int k = 1; k <= shells; ++k) numerator += run_sums[2 * (k - 1)] + run_sums[2 * (k - 1) + 1];
            out[c] = numerator / div_denominator(cut[c], len);
        }
    }
}

}
