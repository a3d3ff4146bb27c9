// Host side of the general sparse-constraint path (csr.hpp): the one-time symbolic analysis and the
// launch sequences.  No numeric work happens here.
#include "csr.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>

namespace po {

namespace {

constexpr int kFrontMin = 16;  // shortest chain scheduled as a front

int internal_error(const char *what) {
  set_error("internal: sparse Cholesky analysis: %s", what);
  return PO_ERR_ARG;
}

constexpr int kNdLeaf = 8;  // subsets this small are numbered as they come

// Nested dissection from BFS level structures (George's automatic nested dissection): the middle
// level of a rooted level structure from a pseudo-peripheral vertex separates the graph; the two
// halves are numbered first, the separator last.  adj is the graph of S without the diagonal.
struct Dissector {
  const std::vector<int> &adjp, &adj;
  std::vector<int> region;  // current subset id of every vertex (-1 = already numbered)
  std::vector<int> level;
  std::vector<int> perm;    // perm[new] = old
  int next_region = 1;

  Dissector(const std::vector<int> &ap, const std::vector<int> &a, int w)
      : adjp(ap), adj(a), region(w, 0), level(w, -1), perm(w, -1) {}

  // BFS inside `reg` from `start`; vertices in visit order into out, level[] filled; returns #levels
  int bfs(int start, int reg, std::vector<int> &out, int stamp_region) {
    out.clear();
    out.push_back(start);
    region[start] = stamp_region;
    level[start] = 0;
    size_t head = 0;
    int nlev = 1;
    while (head < out.size()) {
      const int v = out[head++];
      for (int p = adjp[v]; p < adjp[v + 1]; p++) {
        const int u = adj[p];
        if (region[u] != reg) continue;
        region[u] = stamp_region;
        level[u] = level[v] + 1;
        nlev = level[u] + 1;
        out.push_back(u);
      }
    }
    return nlev;
  }

  void number(const std::vector<int> &verts, int lo) {
    for (size_t i = 0; i < verts.size(); i++) {
      perm[lo + (int)i] = verts[i];
      region[verts[i]] = -1;
    }
  }

  // number the vertices of `verts` (all carrying region id `reg`) into positions [lo, lo + |verts|)
  void order(std::vector<int> &verts, int reg, int lo, int depth) {
    if ((int)verts.size() <= kNdLeaf || depth > 96) {
      number(verts, lo);
      return;
    }
    // connected components first: removing a separator may have split the subset
    std::vector<int> comp, queue;
    std::vector<std::vector<int>> big;
    std::vector<int> big_reg;
    std::vector<int> small;
    for (size_t s = 0; s < verts.size(); s++) {
      if (region[verts[s]] != reg) continue;
      const int r = next_region++;
      bfs(verts[s], reg, comp, r);
      if ((int)comp.size() <= kNdLeaf) {
        small.insert(small.end(), comp.begin(), comp.end());
      } else {
        big.push_back(comp);
        big_reg.push_back(r);
      }
    }
    std::vector<int>().swap(verts);
    number(small, lo);
    lo += (int)small.size();
    for (size_t b = 0; b < big.size(); b++) {
      const int sz = (int)big[b].size();
      bisect(big[b], big_reg[b], lo, depth);
      lo += sz;
    }
  }

  void bisect(std::vector<int> &comp, int reg, int lo, int depth) {
    // pseudo-peripheral start: the last vertex of a BFS, twice
    std::vector<int> lv;
    int r1 = next_region++;
    bfs(comp[0], reg, lv, r1);
    int r2 = next_region++;
    bfs(lv.back(), r1, lv, r2);
    int r3 = next_region++;
    const int nlev = bfs(lv.back(), r2, lv, r3);
    if (nlev < 3) {  // clique-like: nothing to separate
      number(lv, lo);
      return;
    }
    std::vector<int> count(nlev, 0);
    for (int v : lv) count[level[v]]++;
    const int total = (int)lv.size();
    int mid = 1, cum = count[0];
    while (mid < nlev - 2 && cum + count[mid] < total / 2) cum += count[mid++];
    // vertices of the middle level without a neighbour in the next level can stay in the first half
    std::vector<int> A, B, S;
    const int ra = next_region++, rb = next_region++;
    for (int v : lv) {
      const int l = level[v];
      if (l < mid) {
        A.push_back(v);
      } else if (l > mid) {
        B.push_back(v);
      } else {
        bool touches = false;
        for (int p = adjp[v]; p < adjp[v + 1] && !touches; p++) {
          const int u = adj[p];
          touches = region[u] == r3 && level[u] == mid + 1;
        }
        (touches ? S : A).push_back(v);
      }
    }
    for (int v : A) region[v] = ra;
    for (int v : B) region[v] = rb;
    const int na = (int)A.size(), nb = (int)B.size();
    number(S, lo + na + nb);
    std::vector<int>().swap(lv);
    std::vector<int>().swap(comp);
    order(A, ra, lo, depth + 1);
    order(B, rb, lo + na, depth + 1);
  }
};

}  // namespace

// The three steps of the analysis that do not depend on where the graph came from (csr.hpp); the multifrontal
// analysis of sparse_chol.cpp calls the same ones.
void sym_nd_order(const std::vector<int> &adjp, const std::vector<int> &adj, int w, std::vector<int> *perm) {
  Dissector nd(adjp, adj, w);
  std::vector<int> all(w);
  std::iota(all.begin(), all.end(), 0);
  nd.order(all, 0, 0, 0);
  perm->swap(nd.perm);
}

// elimination tree (Liu, with path compression)
void sym_etree(const std::vector<int> &adjp, const std::vector<int> &adj, const std::vector<int> &perm,
               const std::vector<int> &iperm, std::vector<int> *parent_out) {
  const int w = (int)perm.size();
  std::vector<int> &parent = *parent_out;
  parent.assign(w, -1);
  std::vector<int> anc(w, -1);
  for (int i = 0; i < w; i++) {
    const int old = perm[i];
    for (int p = adjp[old]; p < adjp[old + 1]; p++) {
      int r = iperm[adj[p]];
      if (r >= i) continue;
      while (anc[r] != -1 && anc[r] != i) {
        const int nx = anc[r];
        anc[r] = i;
        r = nx;
      }
      if (anc[r] == -1) {
        anc[r] = i;
        parent[r] = i;
      }
    }
  }
}

// entries of every column of L, the diagonal included
void sym_colcount(const std::vector<int> &adjp, const std::vector<int> &adj, const std::vector<int> &perm,
                  const std::vector<int> &iperm, const std::vector<int> &parent, std::vector<int> *colcount_out) {
  const int w = (int)perm.size();
  std::vector<int> &colcount = *colcount_out;
  colcount.assign(w, 1);
  std::vector<int> mark(w, -1);
  for (int i = 0; i < w; i++) {
    const int old = perm[i];
    mark[i] = i;
    for (int p = adjp[old]; p < adjp[old + 1]; p++) {
      int j = iperm[adj[p]];
      if (j >= i) continue;
      while (mark[j] != i) {
        colcount[j]++;
        mark[j] = i;
        j = parent[j];
      }
    }
  }
}

static int csr_analyse_impl(int64_t n64, int64_t w64, const int *rowp, const int *cols, CsrSymbolic *out,
                            bool allow_fronts, int64_t min_rows, int factor_kind);

int csr_analyse(int64_t n, int64_t w, const int *rowp, const int *cols, CsrSymbolic *out, int64_t min_rows,
                int factor_kind) {
  if (factor_kind != PO_SPARSE_FACTOR_ROWS && factor_kind != PO_SPARSE_FACTOR_MULTIFRONTAL) {
    set_error("sparse Jacobian: unknown sparse factor kind %d", factor_kind);
    return PO_ERR_ARG;
  }
  int rc = csr_analyse_impl(n, w, rowp, cols, out, dbg_switch(SW_NO_FRONTS) <= 0, min_rows, factor_kind);
  if (rc == PO_ERR_NUMERIC) {  // a chain that is not a dense front after all: schedule row by row
    *out = CsrSymbolic();
    rc = csr_analyse_impl(n, w, rowp, cols, out, false, min_rows, factor_kind);
  }
  return rc;
}

// The multifrontal factor (csr.hpp: CsrSymbolic) of the matrix whose graph is adjp / adj: the engine's own analysis of
// S0 with its nested dissection, its order taken over, and the entry list of lower(P S0 P^T) composed with the
// engine's value scatter into offsets in its L.
static int analyse_multifrontal(CsrSymbolic &s, const std::vector<int> &adjp, const std::vector<int> &adj) {
  const int w = s.w;
  // S0 in compressed columns, rows ascending, BOTH triangles as the engine's callers pass a matrix: its scatter reads
  // the copy of an entry that lies in the lower triangle AFTER the permutation, which may be either one (the order is
  // the one lower(S0) alone gives: the analysis symmetrises the pattern)
  if (adj.size() + (size_t)w > 2000000000ULL) {
    set_error("sparse Jacobian: Aw Aw^T has more than 2e9 entries, more than the multifrontal factor takes");
    return PO_ERR_ARG;
  }
  std::vector<int> colp((size_t)w + 1, 0), rows;
  rows.reserve(adj.size() + (size_t)w);
  for (int j = 0; j < w; j++) {
    const size_t begin = rows.size();
    rows.push_back(j);
    rows.insert(rows.end(), adj.begin() + adjp[j], adj.begin() + adjp[j + 1]);
    std::sort(rows.begin() + begin, rows.end());
    colp[j + 1] = (int)rows.size();
  }
  PO_TRY(chol_analyse(w, colp.data(), rows.data(), PO_ORDER_ND, nullptr, &s.chol));
  s.factor_kind = PO_SPARSE_FACTOR_MULTIFRONTAL;
  s.perm = s.chol.perm;
  s.iperm = s.chol.iperm;
  s.nnzL = s.chol.nnzL;
  // every destination of the engine's scatter has one source: the copy of the entry that it reads
  std::vector<int64_t> off(rows.size(), -1);
  for (size_t d = 0; d < s.chol.asm_dst.size(); d++) {
    if (s.chol.asm_ptr[d + 1] - s.chol.asm_ptr[d] != 1) return internal_error("an entry of S shares its place in L");
    off[s.chol.asm_src[s.chol.asm_ptr[d]]] = s.chol.asm_dst[d];
  }
  // (column by column, rows ascending: already the order of Aw's rows that the assembly wants, see below)
  const size_t ne = s.chol.asm_dst.size();
  if ((int64_t)ne != s.nnzS) return internal_error("the scatter does not cover lower(S)");
  s.ent_a.clear();
  s.ent_b.clear();
  s.ent_off.clear();
  s.ent_a.reserve(ne);
  s.ent_b.reserve(ne);
  s.ent_off.reserve(ne);
  for (int j = 0; j < w; j++) {
    for (int p = colp[j]; p < colp[j + 1]; p++) {
      if (off[p] < 0) continue;  // the mirror image is the one that is read
      if (off[p] >= s.chol.Lsize) return internal_error("an entry of S has no place in L");
      s.ent_a.push_back(j);
      s.ent_b.push_back(rows[p]);
      s.ent_off.push_back(off[p]);
    }
  }
  s.dense_pos.resize(s.dense_rows.size());
  for (size_t q = 0; q < s.dense_rows.size(); q++) s.dense_pos[q] = s.iperm[s.dense_rows[q]];
  return PO_OK;
}

static int csr_analyse_impl(int64_t n64, int64_t w64, const int *rowp, const int *cols, CsrSymbolic *out,
                            bool allow_fronts, int64_t min_rows, int factor_kind) {
  CsrSymbolic &s = *out;
  if (w64 < 0 || n64 < 0 || w64 > 2000000000LL || n64 > 2000000000LL) {
    set_error("sparse Jacobian: sizes out of range (nwcon %lld, nvars %lld)", (long long)w64, (long long)n64);
    return PO_ERR_ARG;
  }
  const int w = (int)w64, n = (int)n64;
  s.w = w;
  s.n = n;
  if (rowp[0] != 0) {
    set_error("sparse Jacobian: rowp[0] must be 0");
    return PO_ERR_ARG;
  }
  for (int i = 0; i < w; i++) {
    if (rowp[i + 1] < rowp[i]) {
      set_error("sparse Jacobian: rowp is not non-decreasing at row %d", i);
      return PO_ERR_ARG;
    }
  }
  const int nnz = rowp[w];
  s.nnz = nnz;
  // column-sorted rows, remembering the user's slot
  s.rowp.assign(rowp, rowp + w + 1);
  s.cols.resize(nnz);
  s.src.resize(nnz);
  s.identity_src = true;
  {
    std::vector<std::pair<int, int>> row;
    for (int i = 0; i < w; i++) {
      row.clear();
      for (int p = rowp[i]; p < rowp[i + 1]; p++) {
        if (cols[p] < 0 || cols[p] >= n) {
          set_error("sparse Jacobian: column %d out of range in row %d", cols[p], i);
          return PO_ERR_ARG;
        }
        row.push_back(std::make_pair(cols[p], p));
      }
      std::sort(row.begin(), row.end());
      for (size_t q = 0; q < row.size(); q++) {
        if (q > 0 && row[q].first == row[q - 1].first) {
          set_error("sparse Jacobian: column %d appears twice in row %d", row[q].first, i);
          return PO_ERR_ARG;
        }
        const int p = rowp[i] + (int)q;
        s.cols[p] = row[q].first;
        s.src[p] = row[q].second;
        if (row[q].second != p) s.identity_src = false;
      }
    }
  }
  // transpose
  s.colp.assign((size_t)n + 1, 0);
  for (int p = 0; p < nnz; p++) s.colp[s.cols[p] + 1]++;
  double pairs = 0.0;
  for (int j = 0; j < n; j++) {
    const double cnt = s.colp[j + 1];
    pairs += cnt * cnt;
  }
  // The dense-column rule (csr.hpp).  A qualifying column leaves the transposed index, and with it the pattern of
  // S, the ordering and the factor; its entries are recorded on their own.
  int64_t dense_from = 0;  // 0: no column is taken out
  if (min_rows > 0) {
    dense_from = min_rows;
  } else if (min_rows == 0 && pairs > 1.5e9) {
    dense_from = std::max<int64_t>(1024, w / 8);
  }
  s.dense_cols.clear();
  s.dense_ptr.assign(1, 0);
  long long qualified = 0;
  if (dense_from > 0) {
    for (int j = 0; j < n; j++) qualified += s.colp[j + 1] >= dense_from ? 1 : 0;
    if (qualified > kMaxDenseCols) {
      set_error("sparse Jacobian: %lld columns qualify as dense (at least %lld entries each), more than the %d a "
                "low-rank correction takes", qualified, (long long)dense_from, kMaxDenseCols);
      return PO_ERR_ARG;
    }
    for (int j = 0; j < n; j++) {
      const int cnt = s.colp[j + 1];
      if (cnt < dense_from) continue;
      pairs -= (double)cnt * cnt;
      s.dense_cols.push_back(j);
      s.dense_ptr.push_back(s.dense_ptr.back() + cnt);
      s.colp[j + 1] = 0;
    }
  }
  if (pairs > 1.5e9) {
    if (dense_from > 0) {
      set_error("sparse Jacobian: Aw Aw^T would have more than 1.5e9 entries (a dense column?) after %lld columns "
                "with at least %lld entries qualified as dense and were taken out", qualified, (long long)dense_from);
    } else {
      set_error("sparse Jacobian: Aw Aw^T would have more than 1.5e9 entries (a dense column?)");
    }
    return PO_ERR_ARG;
  }
  for (int j = 0; j < n; j++) s.colp[j + 1] += s.colp[j];
  s.rowsT.resize(s.colp[n]);
  s.srcT.resize(s.colp[n]);
  s.dense_rows.resize(s.dense_ptr.back());
  s.dense_slot.resize(s.dense_ptr.back());
  {
    std::vector<int> fill(s.colp.begin(), s.colp.end() - 1);
    std::vector<int> dense_of, dfill(s.dense_ptr.begin(), s.dense_ptr.end() - 1);
    if (!s.dense_cols.empty()) {
      dense_of.assign(n, -1);
      for (size_t j = 0; j < s.dense_cols.size(); j++) dense_of[s.dense_cols[j]] = (int)j;
    }
    for (int i = 0; i < w; i++) {
      for (int p = s.rowp[i]; p < s.rowp[i + 1]; p++) {
        const int jd = dense_of.empty() ? -1 : dense_of[s.cols[p]];
        if (jd >= 0) {
          const int q = dfill[jd]++;
          s.dense_rows[q] = i;
          s.dense_slot[q] = p;
          continue;
        }
        const int q = fill[s.cols[p]]++;
        s.rowsT[q] = i;
        s.srcT[q] = p;
      }
    }
  }
  // graph of S = pattern(Aw Aw^T) without the diagonal
  std::vector<int> adjp((size_t)w + 1, 0), adj;
  {
    std::vector<int> mark(w, -1);
    for (int i = 0; i < w; i++) {
      mark[i] = i;
      for (int p = s.rowp[i]; p < s.rowp[i + 1]; p++) {
        const int k = s.cols[p];
        for (int q = s.colp[k]; q < s.colp[k + 1]; q++) {
          const int j = s.rowsT[q];
          if (mark[j] != i) {
            mark[j] = i;
            adj.push_back(j);
          }
        }
      }
      adjp[i + 1] = (int)adj.size();
    }
  }
  s.nnzS = (int64_t)(adj.size() / 2) + w;
  if (factor_kind == PO_SPARSE_FACTOR_MULTIFRONTAL) return analyse_multifrontal(s, adjp, adj);
  // ordering
  sym_nd_order(adjp, adj, w, &s.perm);
  // The dissection ordering fixes the elimination TREE; any topological order of that tree gives the same
  // factor up to a relabelling.  Rows are renumbered level by level (a row's level = the height of its
  // subtree), so the rows a launch works on - and their storage in L - are contiguous in memory.
  auto invert = [&](const std::vector<int> &perm, std::vector<int> &iperm) -> bool {
    iperm.assign(w, -1);
    for (int i = 0; i < w; i++) {
      if (perm[i] < 0 || perm[i] >= w || iperm[perm[i]] != -1) return false;
      iperm[perm[i]] = i;
    }
    return true;
  };
  auto etree = [&](const std::vector<int> &perm, const std::vector<int> &iperm, std::vector<int> &parent) {
    sym_etree(adjp, adj, perm, iperm, &parent);
  };
  auto levels_of = [&](const std::vector<int> &parent, std::vector<int> &lev) -> int {
    lev.assign(w, 0);
    int nlev = w > 0 ? 1 : 0;
    for (int i = 0; i < w; i++) {
      const int p = parent[i];
      if (p >= 0 && lev[p] < lev[i] + 1) lev[p] = lev[i] + 1;
      if (lev[i] + 1 > nlev) nlev = lev[i] + 1;
    }
    return nlev;
  };
  if (!invert(s.perm, s.iperm)) {
    set_error("internal: ordering is not a permutation");
    return PO_ERR_ARG;
  }
  // Fronts.  A separator of the dissection is a clique, i.e. a chain j -> j+1 -> ... of the tree whose
  // columns have nested structures (a fundamental supernode): row by row it would cost one level per
  // vertex.  Chains of at least kFrontMin rows become FRONTS: one scheduling unit whose rows are numbered
  // consecutively; the part of those rows left of the front is computed for all rows at once, the dense
  // lower triangle inside the front (the tails of the rows) by one workgroup.  Levels are heights in the
  // tree of units.
  std::vector<int> lev(w, 0), front_of(w, -1);
  {
    etree(s.perm, s.iperm, s.parent);
    const std::vector<int> &parent = s.parent;
    std::vector<int> colcount, nchild(w, 0), head(w);
    sym_colcount(adjp, adj, s.perm, s.iperm, parent, &colcount);
    for (int i = 0; i < w; i++) {
      if (parent[i] >= 0) nchild[parent[i]]++;
    }
    std::iota(head.begin(), head.end(), 0);
    if (allow_fronts) {
      for (int j = 0; j + 1 < w; j++) {
        if (parent[j] == j + 1 && nchild[j + 1] == 1 && colcount[j] == colcount[j + 1] + 1) head[j + 1] = head[j];
      }
    }
    std::vector<int> fsize(w, 0), ulev(w, 0);
    for (int i = 0; i < w; i++) fsize[head[i]]++;
    auto unit = [&](int i) { return fsize[head[i]] >= kFrontMin ? head[i] : i; };
    int nlev = w > 0 ? 1 : 0;
    for (int i = 0; i < w; i++) {
      const int u = unit(i), p = parent[i];
      if (ulev[u] + 1 > nlev) nlev = ulev[u] + 1;
      if (p >= 0) {
        const int up = unit(p);
        if (up != u && ulev[up] < ulev[u] + 1) ulev[up] = ulev[u] + 1;
      }
    }
    // bucket (level, ordinary | front), rows ascending inside a bucket: a front stays contiguous
    std::vector<int> start((size_t)2 * nlev + 1, 0), byLevel(w), newlev(w), newfront(w, -1);
    for (int i = 0; i < w; i++) start[2 * ulev[unit(i)] + (fsize[head[i]] >= kFrontMin ? 1 : 0) + 1]++;
    for (int b = 0; b < 2 * nlev; b++) start[b + 1] += start[b];
    std::vector<int> newpos(w);
    for (int i = 0; i < w; i++) {
      const int u = unit(i);
      const bool in_front = fsize[head[i]] >= kFrontMin;
      const int pos = start[2 * ulev[u] + (in_front ? 1 : 0)]++;
      newpos[i] = pos;
      byLevel[pos] = s.perm[i];
      newlev[pos] = ulev[u];
      if (in_front) newfront[pos] = newpos[head[i]];
    }
    s.perm.swap(byLevel);
    lev.swap(newlev);
    front_of.swap(newfront);
    invert(s.perm, s.iperm);
  }
  etree(s.perm, s.iperm, s.parent);
  s.Lrowp.assign((size_t)w + 1, 0);
  s.Lcols.clear();
  {
    std::vector<int> mark(w, -1);
    for (int i = 0; i < w; i++) {
      const int old = s.perm[i];
      const size_t begin = s.Lcols.size();
      mark[i] = i;
      for (int p = adjp[old]; p < adjp[old + 1]; p++) {
        int j = s.iperm[adj[p]];
        if (j >= i) continue;
        while (mark[j] != i) {
          s.Lcols.push_back(j);
          mark[j] = i;
          j = s.parent[j];
        }
      }
      std::sort(s.Lcols.begin() + begin, s.Lcols.end());
      s.Lcols.push_back(i);
      if (s.Lcols.size() > 2000000000ULL) {
        set_error("sparse Cholesky: the factor would have more than 2e9 entries");
        return PO_ERR_ARG;
      }
      s.Lrowp[i + 1] = (int)s.Lcols.size();
    }
  }
  s.nnzL = (int64_t)s.Lcols.size();
  // columns of L below the diagonal
  s.Ltp.assign((size_t)w + 1, 0);
  for (int i = 0; i < w; i++) {
    for (int p = s.Lrowp[i]; p < s.Lrowp[i + 1] - 1; p++) s.Ltp[s.Lcols[p] + 1]++;
  }
  for (int j = 0; j < w; j++) s.Ltp[j + 1] += s.Ltp[j];
  s.Ltrows.resize(s.Ltp[w]);
  s.Ltsrc.resize(s.Ltp[w]);
  {
    std::vector<int> fill(s.Ltp.begin(), s.Ltp.end() - 1);
    for (int i = 0; i < w; i++) {
      for (int p = s.Lrowp[i]; p < s.Lrowp[i + 1] - 1; p++) {
        const int q = fill[s.Lcols[p]]++;
        s.Ltrows[q] = i;
        s.Ltsrc[q] = p;
      }
    }
  }
  // structural entries of lower(P S P^T) -> slot in L
  s.ent_a.clear();
  s.ent_b.clear();
  s.ent_slot.clear();
  for (int i = 0; i < w; i++) {
    const int old = s.perm[i];
    s.ent_a.push_back(old);
    s.ent_b.push_back(old);
    s.ent_slot.push_back(s.Lrowp[i + 1] - 1);
    for (int p = adjp[old]; p < adjp[old + 1]; p++) {
      const int j = s.iperm[adj[p]];
      if (j >= i) continue;
      const int *b = &s.Lcols[s.Lrowp[i]], *e = &s.Lcols[s.Lrowp[i + 1] - 1];
      const int *f = std::lower_bound(b, e, j);
      if (f == e || *f != j) {
        set_error("internal: entry (%d,%d) of S missing from the factor pattern", i, j);
        return PO_ERR_ARG;
      }
      s.ent_a.push_back(old);
      s.ent_b.push_back(adj[p]);
      s.ent_slot.push_back((int)(f - &s.Lcols[0]));
    }
  }
  // assemble in the order of Aw's rows: the (many) reads of an entry walk Aw coalesced, its one write scatters
  {
    const size_t ne = s.ent_slot.size();
    std::vector<int> idx(ne);
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int x, int y) {
      return s.ent_a[x] != s.ent_a[y] ? s.ent_a[x] < s.ent_a[y] : s.ent_b[x] < s.ent_b[y];
    });
    std::vector<int> ta(ne), tb(ne), ts(ne);
    for (size_t k = 0; k < ne; k++) {
      ta[k] = s.ent_a[idx[k]];
      tb[k] = s.ent_b[idx[k]];
      ts[k] = s.ent_slot[idx[k]];
    }
    s.ent_a.swap(ta);
    s.ent_b.swap(tb);
    s.ent_slot.swap(ts);
  }
  // Levels.  An ordinary row needs every row in its pattern, all of them in earlier levels; the rows of a
  // front need earlier levels for the columns left of the front and each other inside it.  The same sets in
  // DESCENDING order schedule the backward solve (x_i needs x_j for the ancestors j in column i).
  {
    int nlev = 0;
    for (int i = 0; i < w; i++) nlev = std::max(nlev, lev[i] + 1);
    s.fwd_ptr.assign((size_t)nlev + 1, 0);
    for (int i = 0; i < w; i++) s.fwd_ptr[lev[i] + 1]++;
    for (int l = 0; l < nlev; l++) s.fwd_ptr[l + 1] += s.fwd_ptr[l];
    s.fwd_order.resize(w);
    std::iota(s.fwd_order.begin(), s.fwd_order.end(), 0);
    s.fwd_maxlen.assign(nlev, 0);
    s.bwd_maxlen.assign(nlev, 0);
    s.ord_end.assign(nlev, 0);
    s.front_ptr.assign((size_t)nlev + 1, 0);
    s.front_maxdesc.assign(nlev, 0);
    s.front_start.clear();
    s.front_size.clear();
    s.front_of = front_of;
    for (int l = 0; l < nlev; l++) {
      int i = s.fwd_ptr[l];
      const int e = s.fwd_ptr[l + 1];
      while (i < e && front_of[i] < 0) {
        if (lev[i] != l) return internal_error("rows are not numbered level by level");
        s.fwd_maxlen[l] = std::max(s.fwd_maxlen[l], s.Lrowp[i + 1] - s.Lrowp[i]);
        s.bwd_maxlen[l] = std::max(s.bwd_maxlen[l], s.Ltp[i + 1] - s.Ltp[i]);
        for (int p = s.Lrowp[i]; p < s.Lrowp[i + 1] - 1; p++) {
          if (lev[s.Lcols[p]] >= l) return internal_error("a row depends on a row of its own level");
        }
        i++;
      }
      s.ord_end[l] = i;
      while (i < e) {
        const int f0 = i;
        if (front_of[i] != f0) return internal_error("front rows are not contiguous");
        int sz = 0;
        while (i < e && front_of[i] == f0) {
          // the tail of row f0 + sz must be exactly the columns f0 .. f0 + sz
          const int len = s.Lrowp[i + 1] - s.Lrowp[i];
          if (lev[i] != l || len < sz + 1 || s.Lcols[s.Lrowp[i + 1] - 1 - sz] != f0) return PO_ERR_NUMERIC;
          for (int p = s.Lrowp[i]; p < s.Lrowp[i + 1] - 1 - sz; p++) {
            if (lev[s.Lcols[p]] >= l) return internal_error("a front depends on a row of its own level");
          }
          s.front_maxdesc[l] = std::max(s.front_maxdesc[l], len - sz - 1);
          sz++;
          i++;
        }
        s.front_start.push_back(f0);
        s.front_size.push_back(sz);
        s.max_front = std::max(s.max_front, sz);
      }
      s.front_ptr[l + 1] = (int)s.front_start.size();
    }
  }
  s.dense_pos.resize(s.dense_rows.size());
  for (size_t q = 0; q < s.dense_rows.size(); q++) s.dense_pos[q] = s.iperm[s.dense_rows[q]];
  return PO_OK;
}

// ---------------------------------------------------------------------------------------------------
CsrSparse::CsrSparse(Ctx *c, int64_t n_, int64_t w_) : ctx(c), n(n_), w(w_), nnz(0) {}

CsrSparse::~CsrSparse() {
  delete mf;
  if (cw) vec_decref(cw);
}

int CsrSparse::densePartials(int nv) {
  const int r = ndense();
  if (nv <= dense.part_cap) return PO_OK;
  PO_HIP(hipStreamSynchronize(ctx->stream));  // (grows a few times in the life of a pattern)
  dense.part_cap = 0;
  PO_TRY(dense.part.alloc((size_t)dense.nb * r * nv + 4, false));
  PO_TRY(dense.Zd.alloc((size_t)r * nv + 4, false));
  dense.part_cap = nv;
  return PO_OK;
}

static int group_for(double avg) {
  if (avg <= 6.0) return 1;
  if (avg <= 24.0) return 4;
  if (avg <= 96.0) return 16;
  return 64;
}

int CsrSparse::allocUser(const int *rowp, const int *cols) {
  nnz = rowp[w];
  user_rowp.assign(rowp, rowp + w + 1);
  user_cols.assign(cols, cols + nnz);
  PO_HIP(hipSetDevice(ctx->device));
  PO_TRY(data.alloc((size_t)nnz + 4, true));
  vals = data;
  cw = vec_new(ctx, w);
  return cw ? PO_OK : PO_ERR_HIP;
}

int CsrSparse::analyse(const int *rowp, const int *cols) {
  const int rc = csr_analyse(n, w, rowp, cols, &sym, dense_min_rows, factor_kind);
  if (rc != PO_OK) {
    sym = CsrSymbolic();
    return rc;
  }
  PO_HIP(hipSetDevice(ctx->device));
  PO_TRY(d_rowp.upload(sym.rowp));
  PO_TRY(d_cols.upload(sym.cols));
  PO_TRY(d_src.upload(sym.src));
  PO_TRY(d_colp.upload(sym.colp));
  PO_TRY(d_rowsT.upload(sym.rowsT));
  PO_TRY(d_srcT.upload(sym.srcT));
  PO_TRY(d_perm.upload(sym.perm));
  PO_TRY(d_iperm.upload(sym.iperm));
  PO_TRY(d_ent_a.upload(sym.ent_a));
  PO_TRY(d_ent_b.upload(sym.ent_b));
  if (sym.factor_kind == PO_SPARSE_FACTOR_MULTIFRONTAL) {
    // the engine owns the factor and every table of its sweeps; of the row factor nothing is allocated
    mf = new SparseChol(ctx);
    mf->sym = std::move(sym.chol);
    sym.chol = CholSymbolic();
    PO_TRY(mf->upload(true));
    PO_TRY(d_ent_off.upload(sym.ent_off));
  } else {
    PO_TRY(d_Lrowp.upload(sym.Lrowp));
    PO_TRY(d_Lcols.upload(sym.Lcols));
    PO_TRY(d_Ltp.upload(sym.Ltp));
    PO_TRY(d_Ltrows.upload(sym.Ltrows));
    PO_TRY(d_Ltsrc.upload(sym.Ltsrc));
    PO_TRY(d_ent_slot.upload(sym.ent_slot));
    PO_TRY(d_fwd.upload(sym.fwd_order));
    std::vector<int> front_end(sym.front_of.size(), -1);
    for (size_t f = 0; f < sym.front_start.size(); f++) {
      for (int r = 0; r < sym.front_size[f]; r++) front_end[sym.front_start[f] + r] = sym.front_start[f] + sym.front_size[f];
    }
    PO_TRY(d_front_of.upload(sym.front_of));
    PO_TRY(d_front_end.upload(front_end));
    PO_TRY(d_fstart.upload(sym.front_start));
    PO_TRY(d_fsize.upload(sym.front_size));
    PO_TRY(Lvals.alloc((size_t)sym.nnzL + 4, false));
  }
  PO_TRY(ones.alloc((size_t)w + 4, true));
  PO_TRY(wwork.alloc((size_t)w + 4, true));
  PO_TRY(d_flag.alloc(4, false));
  PO_HIP(hipDeviceSynchronize());
  PO_TRY(k_fill(ctx, ones, w, 1.0));
  nlevels_f = mf ? 0 : (int)sym.fwd_ptr.size() - 1;
  spmv_group = group_for(w > 0 ? (double)sym.nnz / (double)w : 0.0);
  // (the transposed index holds the sparse columns alone)
  spmvT_group = group_for(n > 0 ? (double)sym.rowsT.size() / (double)n : 0.0);
  if (const int r = ndense()) {
    dense.nb = dense_dot_blocks(w);
    dense.ld = (w + 3) / 4 * 4 + 4;
    for (int j = 0; j < r; j++) dense.maxlen = std::max(dense.maxlen, sym.dense_ptr[j + 1] - sym.dense_ptr[j]);
    std::vector<unsigned char> mask((size_t)n, 0);
    for (int j : sym.dense_cols) mask[j] = 1;
    PO_TRY(dense.mask.upload(mask));
    PO_TRY(dense.cols.upload(sym.dense_cols));
    PO_TRY(dense.ptr.upload(sym.dense_ptr));
    PO_TRY(dense.pos.upload(sym.dense_pos));
    PO_TRY(dense.slot.upload(sym.dense_slot));
    // Vd: the positions outside the pattern stay zero for good, the others are written by valuesChanged()
    PO_TRY(dense.Vd.alloc((size_t)r * dense.ld, true));
    PO_TRY(dense.Yv.alloc((size_t)r * dense.ld, true));
    PO_TRY(dense.Kfac.alloc((size_t)r * r + 4, true));
    PO_TRY(densePartials(std::max(r, 32)));  // (wider panels grow it once)
    PO_HIP(hipDeviceSynchronize());
  }
  return PO_OK;
}

// vals after the analysis: a separate column-sorted copy when the user's entry order is not the sorted one
int CsrSparse::sortedValues() {
  if (sym.identity_src) return PO_OK;
  PO_TRY(sorted_vals.alloc((size_t)nnz + 4, true));
  vals = sorted_vals;
  return PO_OK;
}

int CsrSparse::setPattern(const int *rowp, const int *cols) {
  PO_TRY(analyse(rowp, cols));  // (first: it is what validates the pattern)
  PO_TRY(allocUser(rowp, cols));
  return sortedValues();
}

int CsrSparse::setPatternLight(const int *rowp, const int *cols) {
  PO_TRY(allocUser(rowp, cols));
  light = true;
  return PO_OK;
}

int CsrSparse::upgradeFromLight() {
  if (!light) return PO_OK;
  // The analysis runs after all.  The user-visible value array `data` (po_problem_get_sparse_jacobian_data hands it
  // out as a borrowed pointer, like the reference's getSparseJacobianData) and the constraint-value vector `cw` are
  // not touched: a caller that cached either keeps a valid pointer, and what the gradient callback just wrote stays
  // in place.  If the analysis fails the object stays light, with both.
  PO_TRY(analyse(user_rowp.data(), user_cols.data()));
  light = false;
  return sortedValues();
}

int CsrSparse::valuesChanged() {
  if (light || nnz == 0) return PO_OK;
  if (vals != data) PO_TRY(k_csr_gather(ctx, vals, data, d_src, nnz));
  return k_dense_scatter(ctx, dense.ptr, dense.pos, dense.slot, vals, ndense(), dense.maxlen, dense.ld, dense.Vd);
}

int CsrSparse::spmv(double alpha, const double *px, double *out) {
  return k_csr_spmv(ctx, spmv_group, d_rowp, d_cols, vals, w, alpha, px, nullptr, 1.0, out, out, nullptr);
}

int CsrSparse::spmvT(double alpha, const double *pzw, double *out) {
  PO_TRY(k_csr_spmvT(ctx, spmvT_group, d_colp, d_rowsT, d_srcT, vals, n, alpha, pzw, out, nullptr, out));
  return denseColumnsOut(false, pzw, d_perm, alpha, out, nullptr, out);
}

int CsrSparse::denseColumnsOut(bool pattern_only, const double *y, const int *idx, double alpha, const double *bx,
                               const double *dscale, double *out) {
  const int r = ndense();
  if (r == 0 || w <= 0) return PO_OK;
  if (pattern_only && !dense.Vind) {  // the indicator of V, made when the first column sum asks for it
    PO_TRY(dense.Vind.alloc((size_t)r * dense.ld, false));
    PO_HIP(hipMemsetAsync(dense.Vind, 0, (size_t)r * dense.ld * sizeof(double), ctx->stream));
    PO_TRY(k_dense_scatter(ctx, dense.ptr, dense.pos, dense.slot, nullptr, r, dense.maxlen, dense.ld, dense.Vind));
  }
  const double *B[1] = {y};
  PO_TRY(k_dense_dot(ctx, pattern_only ? dense.Vind : dense.Vd, dense.ld, r, B, 1, idx, w, dense.part));
  return k_dense_out(ctx, dense.part, dense.nb, r, dense.cols, alpha, bx, dscale, out);
}

int CsrSparse::lowRankStep(double *const *Y, int nv) {
  const int r = ndense();
  if (r == 0 || nv <= 0 || w <= 0) return PO_OK;
  PO_TRY(densePartials(nv));
  PO_TRY(k_dense_dot(ctx, dense.Yv, dense.ld, r, Y, nv, nullptr, w, dense.part));
  PO_TRY(k_dense_ksolve(ctx, dense.part, dense.nb, r, nv, dense.Kfac, dense.Zd));
  return k_dense_update(ctx, dense.Yv, dense.ld, r, Y, nv, dense.Zd, w);
}

int CsrSparse::innerProduct(double alpha, const double *cvec, double *out) {
  return k_csr_inner(ctx, d_rowp, d_cols, vals, w, alpha, cvec, out);
}

int CsrSparse::colSum(double scale, const double *y, double *out) {
  if (light) {  // no transposed index was built (setPatternLight): the caller owns the grouped form of this product
    set_error("CsrSparse::colSum on a light (grouped) pattern");
    return PO_ERR_ARG;
  }
  PO_TRY(k_csr_colsum(ctx, d_colp, d_rowsT, n, scale, y, out));
  return denseColumnsOut(true, y, d_perm, scale, nullptr, nullptr, out);
}

int CsrSparse::panelPermuted(const double *d, const double *const *P, int nv, double *const *U) {
  return k_csr_panel(ctx, d_rowp, d_cols, vals, w, d, P, nv, U, d_iperm);
}

int CsrSparse::panelNatural(const double *d, const double *const *P, int nv, double *const *U) {
  return k_csr_panel(ctx, d_rowp, d_cols, vals, w, d, P, nv, U, nullptr);
}

// ---- kernel forms (csr.hpp): every threshold that picks a kernel lives in the functions below ----------------------
static const char *const kFormNames[CF_COUNT] = {
    "level:thin",        "level:table",       "level:search",      "front_rows:table", "front_rows:wide",
    "front_rows:search", "front_syrk:table",  "front_syrk:search", "front_dense:lds",  "front_dense:global",
    "trsv_fwd:thin",     "trsv_fwd:wave",     "trsv_fwd:wave_split", "trsv_bwd:thin",  "trsv_bwd:wave",
    "trsv_bwd:wave_split"};
const char *csr_form_name(int form) { return form >= 0 && form < CF_COUNT ? kFormNames[form] : nullptr; }

// one thread per row when the rows of a level are short, or when there are so many that even long rows keep
// every lane busy; a wavefront per row otherwise
static bool thinLevel(int maxlen, int64_t work_items) { return maxlen <= 24 || (work_items >= 65536 && maxlen <= 96); }

// Capacity of the LDS hash table (csr.hip: RowTable) for rows of at most maxlen entries: a power of two of at least
// twice the row, at most 4096 slots (16 KB of keys + 32 KB of values).  0: the rows are too long, use the search kernels.
static int table_cap(int maxlen) {
  constexpr int kMaxTable = 4096;
  int cap = 64;
  while (cap < 2 * maxlen) cap <<= 1;
  return cap <= kMaxTable ? cap : 0;
}

// a wavefront per (row, right-hand side): with few rows in the level the right-hand sides of a row are spread over
// gridDim.y workgroups of four wavefronts, with many rows one workgroup walks through all of them
static int waveGridY(int nrows, int nv) { return nv > 4 ? (nrows < 1024 ? (nv + 3) / 4 : 1) : 1; }

CsrLevelPlan csr_level_plan(const CsrSymbolic &s, int l, int nv) {
  CsrLevelPlan p;
  const int nord = s.ord_end[l] - s.fwd_ptr[l];
  p.trsv_waves = nv > 1 ? 4 : 1;
  if (nord > 0) {
    if (thinLevel(s.fwd_maxlen[l], nord)) {
      p.level = CF_LEVEL_THIN;
    } else {
      p.level_tcap = table_cap(s.fwd_maxlen[l]);
      p.level = p.level_tcap > 0 ? CF_LEVEL_TABLE : CF_LEVEL_SEARCH;
    }
    if (thinLevel(s.fwd_maxlen[l], (int64_t)nord * nv)) {
      p.trsv_fwd = CF_TRSV_FWD_THIN;
    } else {
      p.fwd_gy = waveGridY(nord, nv);
      p.trsv_fwd = p.fwd_gy > 1 ? CF_TRSV_FWD_WAVE_SPLIT : CF_TRSV_FWD_WAVE;
    }
    if (thinLevel(s.bwd_maxlen[l], (int64_t)nord * nv)) {
      p.trsv_bwd = CF_TRSV_BWD_THIN;
    } else {
      p.bwd_gy = waveGridY(nord, nv);
      p.trsv_bwd = p.bwd_gy > 1 ? CF_TRSV_BWD_WAVE_SPLIT : CF_TRSV_BWD_WAVE;
    }
  }
  if (s.front_ptr[l + 1] > s.front_ptr[l]) {
    const int maxdesc = s.front_maxdesc[l];
    p.front_tcap = table_cap(maxdesc);
    if (p.front_tcap > 0) {
      // long front rows (the top separators): eight wavefronts share each row
      p.front_rows = maxdesc >= 256 ? CF_FRONT_ROWS_WIDE : CF_FRONT_ROWS_TABLE;
      p.front_syrk = CF_FRONT_SYRK_TABLE;
    } else {
      p.front_rows = CF_FRONT_ROWS_SEARCH;
      p.front_syrk = CF_FRONT_SYRK_SEARCH;
    }
    for (int f = s.front_ptr[l]; f < s.front_ptr[l + 1]; f++) {
      (front_in_lds(s.front_size[f]) ? p.front_dense_lds : p.front_dense_global) = true;
    }
  }
  return p;
}

void csr_kernel_forms(const CsrSymbolic &s, int nv, int counts[CF_COUNT]) {
  for (int f = 0; f < CF_COUNT; f++) counts[f] = 0;
  const int nlev = (int)s.fwd_ptr.size() - 1;
  for (int l = 0; l < nlev; l++) {
    bool used[CF_COUNT] = {false};
    for (int j0 = 0; j0 < nv; j0 += csr_slab(nv - j0)) {
      const CsrLevelPlan p = csr_level_plan(s, l, csr_slab(nv - j0));
      for (int f : {p.level, p.front_rows, p.front_syrk, p.trsv_fwd, p.trsv_bwd}) {
        if (f >= 0) used[f] = true;
      }
      if (p.front_dense_lds) used[CF_FRONT_DENSE_LDS] = true;
      if (p.front_dense_global) used[CF_FRONT_DENSE_GLOBAL] = true;
    }
    for (int f = 0; f < CF_COUNT; f++) counts[f] += used[f] ? 1 : 0;
  }
}

int CsrSparse::factor(const double *dinv, const double *cdiag) {
  if (w <= 0) return PO_OK;
  if (mf) {
    // S0 goes straight into the engine's front panels, one thread per structural entry as below; flag[1] starts above
    // every index (the engine keeps the smallest)
    double *L = nullptr;
    PO_TRY(mf->beginAssembly(&L));
    PO_HIP(hipMemsetAsync(d_flag, 0x7f, 4 * sizeof(int), ctx->stream));
    PO_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
    PO_TRY(k_csr_assemble(ctx, d_rowp, d_cols, vals, dinv, cdiag, d_ent_a, d_ent_b, d_ent_off,
                          (int64_t)sym.ent_off.size(), L, dense.mask));
    PO_TRY(mf->factorAssembled(d_flag));
  } else {
    PO_HIP(hipMemsetAsync(Lvals, 0, ((size_t)sym.nnzL + 4) * sizeof(double), ctx->stream));
    PO_HIP(hipMemsetAsync(d_flag, 0, 4 * sizeof(int), ctx->stream));
    PO_TRY(k_csr_assemble(ctx, d_rowp, d_cols, vals, dinv, cdiag, d_ent_a, d_ent_b, d_ent_slot,
                          (int64_t)sym.ent_slot.size(), Lvals, dense.mask));
  }
  for (int l = 0; l < nlevels_f; l++) {
    const int b = sym.fwd_ptr[l], e = sym.fwd_ptr[l + 1];
    const int oe = sym.ord_end[l], f0 = sym.front_ptr[l], nf = sym.front_ptr[l + 1] - f0;
    const CsrLevelPlan plan = csr_level_plan(sym, l, 1);
    PO_TRY(k_chol_level(ctx, d_Lrowp, d_Lcols, Lvals, d_fwd + b, oe - b, d_flag, plan));
    PO_TRY(k_chol_fronts(ctx, d_Lrowp, d_Lcols, Lvals, oe, e - oe, d_front_of, d_fstart + f0, d_fsize + f0, nf,
                         plan, d_flag));
  }
  if (const int r = ndense()) {
    // Yv = L^-1 P V, T = Yv^T Yv, K = E^-1 + T = Lk Lk^T: all queued ahead of the one flag read below
    PO_HIP(hipMemcpyAsync(dense.Yv, dense.Vd, (size_t)r * dense.ld * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    std::vector<double *> cols((size_t)r);
    for (int j = 0; j < r; j++) cols[j] = dense.Yv + (int64_t)j * dense.ld;
    PO_TRY(solveInPlace(cols.data(), r, true, false));
    PO_TRY(k_dense_dot(ctx, dense.Yv, dense.ld, r, cols.data(), r, nullptr, w, dense.part));
    PO_TRY(k_dense_kfactor(ctx, dense.part, dense.nb, r, dinv, dense.cols, dense.Kfac, d_flag, w));
  }
  int flag[4] = {0, 0, 0, 0};
  PO_HIP(hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
  PO_HIP(hipStreamSynchronize(ctx->stream));
  if (flag[0] != 0) {
    // S is not numerically SPD: D^-1 or C has a non-positive entry (an indefinite diagonal Hessian, say).
    // The reference ignores LAPACK's info in the same situation (ParOptSparseCholesky.cpp:631, and the return
    // value of mat->factor at ParOptInteriorPoint.cpp:1930) and carries on with whatever the factor holds;
    // here the offending pivots were replaced by 1 so the factor stays finite, the event is counted, the text
    // is kept for po_last_error() and the interior point carries on too.  po_quasidef_factor reports it.
    std::vector<double> hd((size_t)n), hc((size_t)w);
    double dmin = 0.0, cmin = 0.0;
    long bad = 0;
    if (hipMemcpy(hd.data(), dinv, hd.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(hc.data(), cdiag, hc.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) {
      dmin = hd.empty() ? 0.0 : hd[0];
      cmin = hc.empty() ? 0.0 : hc[0];
      for (double v : hd) {
        if (!(v == v) || v - v != 0.0) bad++;
        if (v < dmin) dmin = v;
      }
      for (double v : hc) {
        if (!(v == v) || v - v != 0.0) bad++;
        if (v < cmin) cmin = v;
      }
    }
    if (flag[1] >= w) {
      set_error("sparse Cholesky: non-positive pivot in dense column %d of the low-rank correction "
                "(min D^-1 %.3e, min C %.3e, %ld non-finite inputs)", sym.dense_cols[flag[1] - w], dmin, cmin, bad);
    } else {
      set_error("sparse Cholesky: non-positive pivot in row %d of the permuted Schur complement "
                "(min D^-1 %.3e, min C %.3e, %ld non-finite inputs)", flag[1], dmin, cmin, bad);
    }
    if (breakdowns++ == 0 && ctx->rank == 0) {
      fprintf(stderr, "ParOpt warning: sparse Cholesky breakdown, the quasi-definite matrix is not positive "
                      "definite (min D^-1 %.3e, min C %.3e); continuing as the reference does\n", dmin, cmin);
    }
  }
  return PO_OK;
}

int CsrSparse::solveInPlace(double *const *Y, int nv, bool forward, bool backward) {
  if (mf) return w <= 0 || nv <= 0 ? PO_OK : mf->sweep(Y, nv, forward, backward);  // (any nv: its own slabs)
  if (csr_slab(nv) < nv) {  // independent right-hand sides: slabs of one kernel's pointer table
    for (int j0 = 0; j0 < nv; j0 += csr_slab(nv - j0)) PO_TRY(solveInPlace(Y + j0, csr_slab(nv - j0), forward, backward));
    return PO_OK;
  }
  if (w <= 0 || nv <= 0) return PO_OK;
  if (forward) {
    for (int l = 0; l < nlevels_f; l++) {
      const int b = sym.fwd_ptr[l], e = sym.fwd_ptr[l + 1];
      const int oe = sym.ord_end[l], f0 = sym.front_ptr[l], nf = sym.front_ptr[l + 1] - f0;
      const CsrLevelPlan plan = csr_level_plan(sym, l, nv);
      PO_TRY(k_trsv_fwd_level(ctx, d_Lrowp, d_Lcols, Lvals, d_fwd + b, oe - b, Y, nv, plan));
      PO_TRY(k_trsv_fronts_fwd(ctx, d_Lrowp, d_Lcols, Lvals, oe, e - oe, d_front_of, d_fstart + f0, d_fsize + f0,
                               nf, Y, nv, plan));
    }
  }
  if (backward) {
    for (int l = nlevels_f - 1; l >= 0; l--) {
      const int b = sym.fwd_ptr[l], e = sym.fwd_ptr[l + 1];
      const int oe = sym.ord_end[l], f0 = sym.front_ptr[l], nf = sym.front_ptr[l + 1] - f0;
      const CsrLevelPlan plan = csr_level_plan(sym, l, nv);
      PO_TRY(k_trsv_fronts_bwd(ctx, d_Lrowp, d_Ltp, d_Ltrows, d_Ltsrc, Lvals, oe, e - oe, d_front_of, d_front_end,
                               d_fstart + f0, d_fsize + f0, nf, Y, nv, plan));
      PO_TRY(k_trsv_bwd_level(ctx, d_Lrowp, d_Ltp, d_Ltrows, d_Ltsrc, Lvals, d_fwd + b, oe - b, Y, nv, plan));
    }
  }
  return PO_OK;
}

int CsrSparse::halfSolve(double *const *U, int nv) { return solveInPlace(U, nv, true, false); }

int CsrSparse::correction(const double *const *Yp, int nv, const double *alpha, double *out) {
  PO_TRY(k_panel_axpy(ctx, wwork, 0.0, nullptr, 0.0, alpha, Yp, nv, w));
  double *Y[1] = {wwork};
  PO_TRY(solveInPlace(Y, 1, false, true));
  PO_TRY(k_csr_gather(ctx, out, wwork, d_iperm, w));
  return k_scale(ctx, out, w, -1.0);
}

int CsrSparse::applyK0(const double *dinv, const double *bx, const double *bw, double *yx, double *yw) {
  // wwork (elimination order) = bw - Aw (dinv o bx)
  PO_TRY(k_csr_spmv(ctx, spmv_group, d_rowp, d_cols, vals, w, -1.0, bx, dinv, bw ? 1.0 : 0.0, bw, wwork,
                    d_iperm));
  double *Y[1] = {wwork};
  if (ndense() == 0) {
    PO_TRY(solveInPlace(Y, 1, true, true));
  } else {
    PO_TRY(solveInPlace(Y, 1, true, false));
    PO_TRY(lowRankStep(Y, 1));
    PO_TRY(solveInPlace(Y, 1, false, true));
  }
  PO_TRY(k_csr_gather(ctx, yw, wwork, d_iperm, w));
  // yx = dinv o (bx + Aw^T yw); the dense columns take yw where it still lies in the elimination order
  PO_TRY(k_csr_spmvT(ctx, spmvT_group, d_colp, d_rowsT, d_srcT, vals, n, 1.0, yw, bx, dinv, yx));
  return denseColumnsOut(false, wwork, nullptr, 1.0, bx, dinv, yx);
}

int CsrSparse::solvePanel(const double *const *U, int nv, double *const *Yw) {
  if (w <= 0 || nv <= 0) return PO_OK;
  if (csr_slab(nv) < nv) {  // independent columns: slabs of one kernel's pointer table
    for (int j0 = 0; j0 < nv; j0 += csr_slab(nv - j0)) PO_TRY(solvePanel(U + j0, csr_slab(nv - j0), Yw + j0));
    return PO_OK;
  }
  const int64_t ld = (w + 3) / 4 * 4 + 4;
  if (nv > dense.spanel_cap) {
    PO_HIP(hipStreamSynchronize(ctx->stream));  // (grows a few times in the life of a pattern)
    dense.spanel_cap = 0;
    PO_TRY(dense.spanel.alloc((size_t)nv * ld, false));
    dense.spanel_cap = nv;
  }
  std::vector<double *> Y((size_t)nv);
  for (int j = 0; j < nv; j++) Y[j] = dense.spanel + (int64_t)j * ld;
  PO_TRY(k_csr_panel_gather(ctx, Y.data(), U, nv, d_perm, 1.0, w));
  PO_TRY(solveInPlace(Y.data(), nv, true, false));
  PO_TRY(lowRankStep(Y.data(), nv));
  PO_TRY(solveInPlace(Y.data(), nv, false, true));
  return k_csr_panel_gather(ctx, Yw, Y.data(), nv, d_iperm, -1.0, w);
}

const char *CsrSparse::factorInfo() {
  // the fields of ParOptQuasiDefSparseMat::getFactorInfo (src/ParOptSparseMat.cpp:433-450); the row factor has no
  // supernodes, its level and front counts take the supernode column
  char buf[192];
  const double tri = 0.5 * (double)w * ((double)w + 1.0);
  if (mf) {  // the reference's own terms: its factor is supernodal too (src/ParOptSparseMat.cpp:433-450)
    snprintf(buf, sizeof(buf), "n %5lld nsnodes %5d nnz(K) %7lld nnz(L) %7lld nnz(L) / nnz(K) %8.4f sparsity(L) %8.2e",
             (long long)w, mf->sym.nsn, (long long)sym.nnzS, (long long)sym.nnzL,
             sym.nnzS > 0 ? (double)sym.nnzL / (double)sym.nnzS : 0.0, tri > 0 ? (double)sym.nnzL / tri : 0.0);
  } else {
    snprintf(buf, sizeof(buf),
             "n %5lld nlevels %5d nfronts %5d nnz(K) %7lld nnz(L) %7lld nnz(L) / nnz(K) %8.4f sparsity(L) %8.2e",
             (long long)w, nlevels_f, (int)sym.front_start.size(), (long long)sym.nnzS, (long long)sym.nnzL,
             sym.nnzS > 0 ? (double)sym.nnzL / (double)sym.nnzS : 0.0, tri > 0 ? (double)sym.nnzL / tri : 0.0);
  }
  info = buf;
  if (ndense() > 0) info += " ndense " + std::to_string(ndense());
  return info.c_str();
}

}  // namespace po
