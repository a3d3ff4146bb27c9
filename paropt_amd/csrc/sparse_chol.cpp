// Host analysis of the multifrontal sparse Cholesky (sparse_chol.hpp).  Pure host code: nothing here touches the
// device, so analysis-only handles work on a machine without one.
#include "sparse_chol.hpp"

#include <algorithm>
#include <map>
#include <numeric>

#include "csr.hpp"

namespace po {

namespace {

int chol_internal(const char *what) {
  set_error("internal: multifrontal analysis: %s", what);
  return PO_ERR_ARG;
}

// First-fit layout of slots whose lifetimes are known level by level: a front's slot is taken at its own level and
// given back once its parent's level has consumed it.
struct ArenaLayout {
  std::map<int64_t, int64_t> free_;  // offset -> size
  int64_t end = 0;
  int64_t take(int64_t size) {
    if (size == 0) return 0;
    int looked = 0;
    for (auto it = free_.begin(); it != free_.end() && looked < 64; ++it, ++looked) {
      if (it->second >= size) {
        const int64_t off = it->first, rest = it->second - size;
        free_.erase(it);
        if (rest > 0) free_[off + size] = rest;
        return off;
      }
    }
    const int64_t off = end;
    end += size;
    return off;
  }
  void give(int64_t off, int64_t size) {
    if (size == 0) return;
    auto it = free_.emplace(off, size).first;
    auto nx = std::next(it);
    if (nx != free_.end() && it->first + it->second == nx->first) {
      it->second += nx->second;
      free_.erase(nx);
    }
    if (it != free_.begin()) {
      auto pv = std::prev(it);
      if (pv->first + pv->second == it->first) {
        pv->second += it->second;
        free_.erase(it);
      }
    }
  }
};

// position of the permuted entry (pr, pc), pr >= pc, in L's storage; -1 when outside the pattern
int64_t locate(const CholSymbolic &s, int pr, int pc) {
  const int J = s.sn_of[pc], first = s.sn_first[J], sz = s.sn_first[J + 1] - first;
  int64_t row;
  if (pr < first + sz) {
    row = pr - first;
  } else {
    const int *b = s.below_rows.data() + s.rows_ptr[J], *e = s.below_rows.data() + s.rows_ptr[J + 1];
    const int *f = std::lower_bound(b, e, pr);
    if (f == e || *f != pr) return -1;
    row = sz + (f - b);
  }
  return s.panel_off[J] + (int64_t)(pc - first) * s.sn_ld[J] + row;
}

}  // namespace

int chol_scatter_table(const CholSymbolic &s, int64_t n, const int *colp, const int *rows, std::vector<int> *ptr,
                       std::vector<int64_t> *dst, std::vector<int> *src) {
  if (n != s.n || !colp || colp[0] != 0) {
    set_error("sparse Cholesky values: the pattern has size %lld, the factor %d (or colp[0] is not 0)", (long long)n,
              s.n);
    return PO_ERR_ARG;
  }
  std::vector<std::pair<int64_t, int>> ent;
  for (int j = 0; j < s.n; j++) {
    if (colp[j + 1] < colp[j]) {
      set_error("sparse Cholesky values: colp is not non-decreasing at column %d", j);
      return PO_ERR_ARG;
    }
    const int pc = s.iperm[j];
    for (int p = colp[j]; p < colp[j + 1]; p++) {
      const int i = rows[p];
      if (i < 0 || i >= s.n) {
        set_error("sparse Cholesky values: row %d out of range in column %d", i, j);
        return PO_ERR_ARG;
      }
      const int pr = s.iperm[i];
      if (pr < pc) continue;  // the permuted-upper copy is not read (src/ParOptSparseCholesky.cpp:228)
      const int64_t d = locate(s, pr, pc);
      if (d < 0) {
        set_error("sparse Cholesky values: entry (%d, %d) lies outside the pattern the factor was created with", i, j);
        return PO_ERR_ARG;
      }
      ent.push_back(std::make_pair(d, p));
    }
  }
  std::sort(ent.begin(), ent.end());
  ptr->assign(1, 0);
  dst->clear();
  src->resize(ent.size());
  for (size_t k = 0; k < ent.size(); k++) {
    if (k > 0 && ent[k].first != ent[k - 1].first) ptr->push_back((int)k);
    if (k == 0 || ent[k].first != ent[k - 1].first) dst->push_back(ent[k].first);
    (*src)[k] = ent[k].second;
  }
  if (ent.empty()) {
    ptr->assign(1, 0);
  } else {
    ptr->push_back((int)ent.size());
  }
  return PO_OK;
}

void chol_matrix_table(CholSymbolic *out) {
  CholSymbolic &s = *out;
  if (!s.mat_rowp.empty()) return;
  const size_t nd = s.asm_dst.size();
  // the permuted position of destination d, from its first source (every source of d has the same one)
  std::vector<int> pr(nd), pc(nd);
  s.mat_rowp.assign((size_t)s.n + 1, 0);
  for (size_t d = 0; d < nd; d++) {
    const int p = s.asm_src[s.asm_ptr[d]];
    const int j = (int)(std::upper_bound(s.colp.begin(), s.colp.end(), p) - s.colp.begin()) - 1;
    pr[d] = s.iperm[s.rows[p]];
    pc[d] = s.iperm[j];
    s.mat_rowp[pr[d] + 1]++;
    if (pr[d] != pc[d]) s.mat_rowp[pc[d] + 1]++;
  }
  for (int i = 0; i < s.n; i++) s.mat_rowp[i + 1] += s.mat_rowp[i];
  std::vector<std::pair<int, int>> ent((size_t)s.mat_rowp[s.n]);  // (column, value index), row by row
  std::vector<int> next(s.mat_rowp.begin(), s.mat_rowp.end() - 1);
  for (size_t d = 0; d < nd; d++) {
    ent[next[pr[d]]++] = std::make_pair(pc[d], (int)d);
    if (pr[d] != pc[d]) ent[next[pc[d]]++] = std::make_pair(pr[d], (int)d);
  }
  s.mat_col.resize(ent.size());
  s.mat_vidx.resize(ent.size());
  s.mat_long.clear();
  s.mat_maxrow = 0;
  for (int i = 0; i < s.n; i++) {
    std::sort(ent.begin() + s.mat_rowp[i], ent.begin() + s.mat_rowp[i + 1]);
    const int len = s.mat_rowp[i + 1] - s.mat_rowp[i];
    s.mat_maxrow = std::max(s.mat_maxrow, len);
    if (len > kCholLongRow) s.mat_long.push_back(i);
  }
  for (size_t k = 0; k < ent.size(); k++) {
    s.mat_col[k] = ent[k].first;
    s.mat_vidx[k] = ent[k].second;
  }
}

int chol_analyse(int64_t size, const int *colp, const int *rows, int order, const int *user_perm, CholSymbolic *out) {
  return chol_analyse(size, colp, rows, order, user_perm, 0, nullptr, out);
}

namespace {

// The Schur set's part of the ordering (sparse_chol.hpp, "Schur complement"): the ordering type on the graph induced
// on the interior unknowns, the set after it in the caller's order; then adjp / adj get the set as a clique, so the
// elimination tree chains its columns and every A22 entry lies in the pattern.
int schur_order(int n, int order, const int *user_perm, const std::vector<int> &schur, std::vector<int> *adjp_io,
                std::vector<int> *adj_io, std::vector<int> *perm) {
  const std::vector<int> &adjp = *adjp_io, &adj = *adj_io;
  const int ns = (int)schur.size(), ni = n - ns;
  std::vector<int> interior_of(n, 0);  // -1 on the set, else the index among the interior unknowns
  for (int v : schur) interior_of[v] = -1;
  std::vector<int> interior;
  interior.reserve(ni);
  for (int v = 0; v < n; v++) {
    if (interior_of[v] == 0) {
      interior_of[v] = (int)interior.size();
      interior.push_back(v);
    }
  }
  perm->resize(n);
  if (order == PO_ORDER_NATURAL) {
    if (user_perm) {
      for (int k = 0; k < ns; k++) {
        if (user_perm[ni + k] != schur[k]) {
          set_error("sparse Cholesky: with a Schur set, perm must list the set last and in the order given (perm[%d] "
                    "is %d, the set has %d there)", ni + k, user_perm[ni + k], schur[k]);
          return PO_ERR_ARG;
        }
      }
      perm->assign(user_perm, user_perm + n);
    } else {
      std::copy(interior.begin(), interior.end(), perm->begin());
    }
  } else if (ni > 0) {
    std::vector<int> ip((size_t)ni + 1, 0), ia, iperm;
    for (int k = 0; k < ni; k++) {
      const int v = interior[k];
      for (int p = adjp[v]; p < adjp[v + 1]; p++) {
        if (interior_of[adj[p]] >= 0) ia.push_back(interior_of[adj[p]]);  // (ascending: interior_of is monotone)
      }
      ip[k + 1] = (int)ia.size();
    }
    sym_nd_order(ip, ia, ni, &iperm);
    for (int k = 0; k < ni; k++) (*perm)[k] = interior[iperm[k]];
  }
  std::copy(schur.begin(), schur.end(), perm->begin() + ni);
  // the clique
  int64_t total = 0;
  for (int v = 0; v < n; v++) total += interior_of[v] >= 0 ? adjp[v + 1] - adjp[v] : (adjp[v + 1] - adjp[v]) + ns;
  if (total > 2000000000LL) {
    set_error("sparse Cholesky: the pattern with the Schur set as a clique has more than 2e9 entries");
    return PO_ERR_ARG;
  }
  std::vector<int> sorted(schur);
  std::sort(sorted.begin(), sorted.end());
  std::vector<int> np((size_t)n + 1, 0), na;
  na.reserve((size_t)total);
  for (int v = 0; v < n; v++) {
    if (interior_of[v] >= 0) {
      na.insert(na.end(), adj.begin() + adjp[v], adj.begin() + adjp[v + 1]);
    } else {
      const size_t begin = na.size();
      for (int p = adjp[v]; p < adjp[v + 1]; p++) {
        if (interior_of[adj[p]] >= 0) na.push_back(adj[p]);
      }
      const size_t mid = na.size();
      for (int u : sorted) {
        if (u != v) na.push_back(u);
      }
      std::inplace_merge(na.begin() + begin, na.begin() + mid, na.end());
    }
    np[v + 1] = (int)na.size();
  }
  adjp_io->swap(np);
  adj_io->swap(na);
  return PO_OK;
}

// The gather tables of the Schur supernode S (sparse_chol.hpp: schur_*), the children in child order.
void schur_tables(CholSymbolic *out) {
  CholSymbolic &s = *out;
  const int S = s.schur_sn, ns = s.ns, ld = s.sn_ld[S];
  // factorization: count per destination (col, row) of the lower triangle, prefix sum, fill child after child
  std::vector<int64_t> cnt((size_t)ns * ns + 1, 0);
  std::vector<int64_t> vcnt((size_t)ns + 1, 0);
  for (int c = s.child_ptr[S]; c < s.child_ptr[S + 1]; c++) {
    const int C = s.child[c], bc = s.sn_b[C];
    const int *rel = s.rel.data() + s.rows_ptr[C];
    for (int j = 0; j < bc; j++) {
      vcnt[rel[j] + 1]++;
      for (int i = j; i < bc; i++) cnt[(size_t)rel[j] * ns + rel[i] + 1]++;
    }
  }
  for (size_t k = 0; k < (size_t)ns * ns; k++) cnt[k + 1] += cnt[k];
  for (int k = 0; k < ns; k++) vcnt[k + 1] += vcnt[k];
  s.schur_src.assign((size_t)cnt[(size_t)ns * ns], 0);
  s.schur_vsrc.assign((size_t)vcnt[ns], 0);
  s.schur_vld.assign((size_t)vcnt[ns], 0);
  {
    std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1), vfill(vcnt.begin(), vcnt.end() - 1);
    for (int c = s.child_ptr[S]; c < s.child_ptr[S + 1]; c++) {
      const int C = s.child[c], bc = s.sn_b[C], ulc = s.upd_ld[C];
      const int *rel = s.rel.data() + s.rows_ptr[C];
      for (int j = 0; j < bc; j++) {
        const int64_t q = vfill[rel[j]]++;
        s.schur_vsrc[q] = s.sol_off[C] + j;
        s.schur_vld[q] = ulc;
        for (int i = j; i < bc; i++) s.schur_src[fill[(size_t)rel[j] * ns + rel[i]]++] = s.upd_off[C] + (int64_t)j * ulc + i;
      }
    }
  }
  s.schur_vptr.swap(vcnt);
  // keep the destinations that have sources
  s.schur_ptr.assign(1, 0);
  s.schur_dst.clear();
  for (int col = 0; col < ns; col++) {
    for (int row = col; row < ns; row++) {
      const size_t k = (size_t)col * ns + row;
      if (cnt[k + 1] == cnt[k]) continue;
      s.schur_dst.push_back(s.panel_off[S] + (int64_t)col * ld + row);
      s.schur_ptr.push_back(cnt[k + 1]);
    }
  }
}

}  // namespace

int chol_analyse(int64_t size, const int *colp, const int *rows, int order, const int *user_perm, int64_t nschur,
                 const int *schur, CholSymbolic *out) {
  CholSymbolic &s = *out;
  if (size < 0 || size > 2000000000LL) {
    set_error("sparse Cholesky: size %lld out of range", (long long)size);
    return PO_ERR_ARG;
  }
  if (order != PO_ORDER_NATURAL && order != PO_ORDER_AMD && order != PO_ORDER_ND) {
    set_error("sparse Cholesky: unknown ordering type %d", order);
    return PO_ERR_ARG;
  }
  if (!colp || colp[0] != 0) {
    set_error("sparse Cholesky: colp is missing or colp[0] is not 0");
    return PO_ERR_ARG;
  }
  const int n = (int)size;
  for (int j = 0; j < n; j++) {
    if (colp[j + 1] < colp[j]) {
      set_error("sparse Cholesky: colp is not non-decreasing at column %d", j);
      return PO_ERR_ARG;
    }
  }
  if (nschur < 0 || nschur > n || (nschur > 0 && !schur)) {
    set_error("sparse Cholesky: a Schur set of %lld unknowns (size %d), or its indices are missing", (long long)nschur,
              n);
    return PO_ERR_ARG;
  }
  const int ns = (int)nschur;
  s.ns = ns;
  s.schur_sn = -1;
  s.schur.assign(schur, schur + ns);
  if (ns > 0) {
    std::vector<char> seen(n, 0);
    for (int k = 0; k < ns; k++) {
      if (schur[k] < 0 || schur[k] >= n || seen[schur[k]]) {
        set_error("sparse Cholesky: Schur index %d (entry %d of the set) is out of range or repeated", schur[k], k);
        return PO_ERR_ARG;
      }
      seen[schur[k]] = 1;
    }
  }
  const int nnz = colp[n];
  if (nnz > 0 && !rows) {
    set_error("sparse Cholesky: rows is missing");
    return PO_ERR_ARG;
  }
  s.n = n;
  s.order = order;
  s.colp.assign(colp, colp + n + 1);
  s.rows.assign(rows, rows + nnz);
  // graph of A + A^T without the diagonal: sorted, no duplicates
  std::vector<int> adjp((size_t)n + 1, 0), adj;
  {
    std::vector<int64_t> cnt((size_t)n + 1, 0);
    for (int j = 0; j < n; j++) {
      for (int p = colp[j]; p < colp[j + 1]; p++) {
        const int i = rows[p];
        if (i < 0 || i >= n) {
          set_error("sparse Cholesky: row %d out of range in column %d", i, j);
          return PO_ERR_ARG;
        }
        if (i == j) continue;
        cnt[i + 1]++;
        cnt[j + 1]++;
      }
    }
    for (int j = 0; j < n; j++) cnt[j + 1] += cnt[j];
    if (cnt[n] > 2000000000LL) {
      set_error("sparse Cholesky: the symmetrised pattern has more than 2e9 entries");
      return PO_ERR_ARG;
    }
    std::vector<int> raw((size_t)cnt[n]);
    std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
    for (int j = 0; j < n; j++) {
      for (int p = colp[j]; p < colp[j + 1]; p++) {
        const int i = rows[p];
        if (i == j) continue;
        raw[fill[i]++] = j;
        raw[fill[j]++] = i;
      }
    }
    adj.reserve(raw.size() / 2 + 1);
    for (int j = 0; j < n; j++) {
      std::sort(raw.begin() + cnt[j], raw.begin() + cnt[j + 1]);
      for (int64_t p = cnt[j]; p < cnt[j + 1]; p++) {
        if (p == cnt[j] || raw[p] != raw[p - 1]) adj.push_back(raw[p]);
      }
      adjp[j + 1] = (int)adj.size();
    }
  }
  // ordering
  if (ns > 0) {
    if (order == PO_ORDER_NATURAL && user_perm) {  // (checked here: schur_order reads it as a permutation)
      std::vector<char> seen(n, 0);
      for (int i = 0; i < n; i++) {
        if (user_perm[i] < 0 || user_perm[i] >= n || seen[user_perm[i]]) {
          set_error("sparse Cholesky: perm is not a permutation of 0 .. %d", n - 1);
          return PO_ERR_ARG;
        }
        seen[user_perm[i]] = 1;
      }
    }
    PO_TRY(schur_order(n, order, user_perm, s.schur, &adjp, &adj, &s.perm));
  } else if (order == PO_ORDER_NATURAL) {
    s.perm.resize(n);
    if (user_perm) {
      s.perm.assign(user_perm, user_perm + n);
    } else {
      std::iota(s.perm.begin(), s.perm.end(), 0);
    }
  } else {
    sym_nd_order(adjp, adj, n, &s.perm);
  }
  auto invert = [&](const std::vector<int> &perm, std::vector<int> &iperm) -> bool {
    iperm.assign(n, -1);
    for (int i = 0; i < n; i++) {
      if (perm[i] < 0 || perm[i] >= n || iperm[perm[i]] != -1) return false;
      iperm[perm[i]] = i;
    }
    return true;
  };
  if (!invert(s.perm, s.iperm)) {
    set_error("sparse Cholesky: perm is not a permutation of 0 .. %d", n - 1);
    return PO_ERR_ARG;
  }
  // The elimination tree in POSTORDER: the same factor up to a relabelling, and every chain of the tree -- so every
  // supernode -- becomes a run of consecutive columns with its subtree right in front of it.
  std::vector<int> parent, colcount;
  sym_etree(adjp, adj, s.perm, s.iperm, &parent);
  {
    std::vector<int> head(n, -1), next(n, -1);
    for (int j = n - 1; j >= 0; j--) {  // children ascending
      const int p = parent[j];
      if (p >= 0) {
        next[j] = head[p];
        head[p] = j;
      }
    }
    std::vector<int> post, stack;
    post.reserve(n);
    for (int r = 0; r < n; r++) {
      if (parent[r] >= 0) continue;
      stack.push_back(r);
      while (!stack.empty()) {
        const int v = stack.back();
        const int c = head[v];
        if (c >= 0) {
          head[v] = next[c];
          stack.push_back(c);
        } else {
          post.push_back(v);
          stack.pop_back();
        }
      }
    }
    if ((int)post.size() != n) return chol_internal("the elimination tree is not a forest");
    std::vector<int> np(n);
    for (int k = 0; k < n; k++) np[k] = s.perm[post[k]];
    s.perm.swap(np);
    invert(s.perm, s.iperm);
  }
  sym_etree(adjp, adj, s.perm, s.iperm, &parent);
  sym_colcount(adjp, adj, s.perm, s.iperm, parent, &colcount);
  // fundamental supernodes
  s.sn_of.assign(n, 0);
  s.sn_first.clear();
  {
    std::vector<int> nchild(n, 0);
    for (int j = 0; j < n; j++) {
      if (parent[j] >= 0) nchild[parent[j]]++;
    }
    for (int j = 0; j < n; j++) {
      bool joins = j > 0 && parent[j - 1] == j && nchild[j] == 1 && colcount[j - 1] == colcount[j] + 1;
      // the Schur set: a break in front of it, none inside it (whatever attaches at its later columns)
      if (ns > 0 && j >= n - ns) joins = j > n - ns;
      if (!joins) s.sn_first.push_back(j);
      s.sn_of[j] = (int)s.sn_first.size() - 1;
    }
    s.nsn = (int)s.sn_first.size();
    s.sn_first.push_back(n);
    if (ns > 0) {
      s.schur_sn = s.nsn - 1;
      for (int k = 0; k < ns; k++) {
        if (s.perm[n - ns + k] != s.schur[k]) return chol_internal("the postorder moved the Schur set");
      }
    }
  }
  const int nsn = s.nsn;
  // row structures, children first
  s.sn_b.assign(nsn, 0);
  s.sn_parent.assign(nsn, -1);
  s.rows_ptr.assign((size_t)nsn + 1, 0);
  s.below_rows.clear();
  {
    std::vector<int> mark(n, -1), chead(nsn, -1), cnext(nsn, -1), ctail(nsn, -1);
    for (int J = 0; J < nsn; J++) {
      const int first = s.sn_first[J], last = s.sn_first[J + 1] - 1;
      const size_t begin = s.below_rows.size();
      for (int j = first; j <= last; j++) {
        const int old = s.perm[j];
        for (int p = adjp[old]; p < adjp[old + 1]; p++) {
          const int r = s.iperm[adj[p]];
          if (r > last && mark[r] != J) {
            mark[r] = J;
            s.below_rows.push_back(r);
          }
        }
      }
      for (int c = chead[J]; c >= 0; c = cnext[c]) {
        for (int64_t q = s.rows_ptr[c]; q < s.rows_ptr[c + 1]; q++) {
          const int r = s.below_rows[q];
          if (r > last && mark[r] != J) {
            mark[r] = J;
            s.below_rows.push_back(r);
          }
        }
      }
      std::sort(s.below_rows.begin() + begin, s.below_rows.end());
      const int b = (int)(s.below_rows.size() - begin);
      if (b != colcount[first] - (last - first + 1)) return chol_internal("a supernode's rows disagree with its column count");
      s.sn_b[J] = b;
      s.rows_ptr[J + 1] = (int64_t)s.below_rows.size();
      if (b > 0) {
        const int P = s.sn_of[s.below_rows[begin]];
        if (P <= J) return chol_internal("a supernode's parent does not come after it");
        s.sn_parent[J] = P;
        if (chead[P] < 0) {
          chead[P] = J;
        } else {
          cnext[ctail[P]] = J;
        }
        ctail[P] = J;
      }
    }
    s.child_ptr.assign((size_t)nsn + 1, 0);
    s.child.clear();
    for (int J = 0; J < nsn; J++) {
      for (int c = chead[J]; c >= 0; c = cnext[c]) s.child.push_back(c);
      s.child_ptr[J + 1] = (int)s.child.size();
    }
  }
  // relative indices, levels, storage
  s.rel.assign(s.below_rows.size(), 0);
  s.sn_level.assign(nsn, 0);
  s.sn_ld.assign(nsn, 0);
  s.upd_ld.assign(nsn, 0);
  s.panel_off.assign(nsn, 0);
  s.nnzL = 0;
  s.Lsize = 0;
  s.max_s = s.max_front = 0;
  for (int J = 0; J < nsn; J++) {
    const int sz = s.sn_first[J + 1] - s.sn_first[J], b = s.sn_b[J], P = s.sn_parent[J];
    if (P >= 0) {
      const int pf = s.sn_first[P], ps = s.sn_first[P + 1] - pf;
      const int *pb = s.below_rows.data() + s.rows_ptr[P], *pe = s.below_rows.data() + s.rows_ptr[P + 1];
      for (int64_t q = s.rows_ptr[J]; q < s.rows_ptr[J + 1]; q++) {
        const int r = s.below_rows[q];
        if (r < pf + ps) {
          s.rel[q] = r - pf;
        } else {
          const int *f = std::lower_bound(pb, pe, r);
          if (f == pe || *f != r) return chol_internal("a child's row is missing from its parent's front");
          s.rel[q] = ps + (int)(f - pb);
        }
      }
      s.sn_level[P] = std::max(s.sn_level[P], s.sn_level[J] + 1);
    }
    s.sn_ld[J] = (sz + b + 1) / 2 * 2;
    s.upd_ld[J] = (b + 1) / 2 * 2;
    s.panel_off[J] = s.Lsize;
    s.Lsize += (int64_t)s.sn_ld[J] * sz;
    s.nnzL += (int64_t)sz * (sz + 1) / 2 + (int64_t)b * sz;
    s.max_s = std::max(s.max_s, sz);
    s.max_front = std::max(s.max_front, sz + b);
  }
  s.nlev = 0;
  for (int J = 0; J < nsn; J++) s.nlev = std::max(s.nlev, s.sn_level[J] + 1);
  auto order_of = [&](int J) { return s.sn_first[J + 1] - s.sn_first[J] + s.sn_b[J]; };
  auto nblk_of = [&](int J) { return (s.sn_first[J + 1] - s.sn_first[J] + kCholNB - 1) / kCholNB; };
  // packed groups: supernodes are in postorder, so the subtree of J is the range [J - cnt[J] + 1, J]
  s.pack_cap = std::max(0, dbg_switch(SW_CHOL_PACK));
  s.schur_w = std::max(1, dbg_switch(SW_CHOL_SCHUR_W) / kCholNB) * kCholNB;  // (a multiple of the block width)
  s.front_order.resize(nsn);
  for (int J = 0; J < nsn; J++) s.front_order[J] = order_of(J);
  std::vector<int> grp_of(nsn, -1);
  s.grp_first.clear();
  s.grp_root.clear();
  s.grp_level.clear();
  if (s.pack_cap > 0) {
    std::vector<int> cnt(nsn, 1);
    std::vector<char> packable(nsn, 0), cand(nsn, 0);
    for (int J = 0; J < nsn; J++) {
      bool ok = order_of(J) <= kCholTiny && J != s.schur_sn;
      for (int c = s.child_ptr[J]; c < s.child_ptr[J + 1]; c++) {
        cnt[J] += cnt[s.child[c]];
        ok = ok && packable[s.child[c]];
      }
      packable[J] = ok;
      cand[J] = ok && cnt[J] <= s.pack_cap;
    }
    for (int J = 0; J < nsn; J++) {
      const int P = s.sn_parent[J];
      if (cand[J] && !(P >= 0 && cand[P])) {
        for (int K = J - cnt[J] + 1; K <= J; K++) {
          if (grp_of[K] != -1 || (K < J && (s.sn_parent[K] < 0 || s.sn_parent[K] > J)))
            return chol_internal("a supernode's subtree is not the run of supernodes in front of it");
          grp_of[K] = J;  // (the root for now)
        }
      }
    }
    for (int J = 0; J < nsn; J++) {
      if (grp_of[J] == -1 && order_of(J) <= kCholTiny && J != s.schur_sn) grp_of[J] = J;
    }
    for (int J = 0; J < nsn; J++) {
      if (grp_of[J] != J) continue;
      int f = J;
      while (f > 0 && grp_of[f - 1] == J) f--;
      s.grp_first.push_back(f);
      s.grp_root.push_back(J);
      s.grp_level.push_back(s.sn_level[J]);
    }
  }
  const int ngrp = (int)s.grp_root.size();
  s.glev_ptr.assign((size_t)s.nlev + 1, 0);
  for (int g = 0; g < ngrp; g++) s.glev_ptr[s.grp_level[g] + 1]++;
  for (int l = 0; l < s.nlev; l++) s.glev_ptr[l + 1] += s.glev_ptr[l];
  s.glev_first.resize(ngrp);
  s.glev_root.resize(ngrp);
  {
    std::vector<int> fill(s.glev_ptr.begin(), s.glev_ptr.end() - 1);
    for (int g = 0; g < ngrp; g++) {
      const int q = fill[s.grp_level[g]]++;
      s.glev_first[q] = s.grp_first[g];
      s.glev_root[q] = s.grp_root[g];
    }
  }
  // level lists of the unpacked fronts
  s.lev_ptr.assign((size_t)s.nlev + 1, 0);
  for (int J = 0; J < nsn; J++) {
    if (grp_of[J] == -1 && J != s.schur_sn) s.lev_ptr[s.sn_level[J] + 1]++;
  }
  for (int l = 0; l < s.nlev; l++) s.lev_ptr[l + 1] += s.lev_ptr[l];
  s.lev_sn.resize(s.lev_ptr[s.nlev]);
  s.lev_nsmall.assign(s.nlev, 0);
  {
    std::vector<int> fill(s.lev_ptr.begin(), s.lev_ptr.end() - 1);
    for (int J = 0; J < nsn; J++) {
      if (grp_of[J] == -1 && J != s.schur_sn) s.lev_sn[fill[s.sn_level[J]]++] = J;
    }
    for (int l = 0; l < s.nlev; l++) {
      auto b = s.lev_sn.begin() + s.lev_ptr[l], e = s.lev_sn.begin() + s.lev_ptr[l + 1];
      auto mid = std::stable_partition(b, e, [&](int J) { return order_of(J) <= kCholSmall; });
      s.lev_nsmall[l] = (int)(mid - b);
      std::stable_sort(mid, e, [&](int x, int y) { return nblk_of(x) > nblk_of(y); });
    }
  }
  // Arena layouts: update matrices (factorization) and update vectors (forward solve), the same lifetimes.  A slot is
  // taken at the level that launches its front -- a packed front's is the level of its group's root, whose lane both
  // writes and reads the slots inside the group -- and given back once the level of the front's parent is through.
  s.upd_off.assign(nsn, 0);
  s.sol_off.assign(nsn, 0);
  {
    ArenaLayout fa, so;
    auto take = [&](int J) {
      s.upd_off[J] = fa.take((int64_t)s.upd_ld[J] * s.sn_b[J]);
      s.sol_off[J] = so.take((int64_t)s.upd_ld[J] * kCholMaxRhs);
    };
    auto give_children = [&](int J) {
      for (int c = s.child_ptr[J]; c < s.child_ptr[J + 1]; c++) {
        const int C = s.child[c];
        fa.give(s.upd_off[C], (int64_t)s.upd_ld[C] * s.sn_b[C]);
        so.give(s.sol_off[C], (int64_t)s.upd_ld[C] * kCholMaxRhs);
      }
    };
    for (int l = 0; l < s.nlev; l++) {
      for (int q = s.lev_ptr[l]; q < s.lev_ptr[l + 1]; q++) take(s.lev_sn[q]);
      for (int q = s.glev_ptr[l]; q < s.glev_ptr[l + 1]; q++) {
        for (int J = s.glev_first[q]; J <= s.glev_root[q]; J++) take(J);
      }
      for (int q = s.lev_ptr[l]; q < s.lev_ptr[l + 1]; q++) give_children(s.lev_sn[q]);
      for (int q = s.glev_ptr[l]; q < s.glev_ptr[l + 1]; q++) {
        for (int J = s.glev_first[q]; J <= s.glev_root[q]; J++) give_children(J);
      }
      // (the slots of the Schur supernode's children are never given back: its two gathers may then run at any
      // point after its level, and it is the last front of its tree anyway)
    }
    s.arena = fa.end;
    s.sol_arena = so.end;
  }
  s.work_bytes = 8 * (std::max(s.arena, s.sol_arena) + s.ldy() * kCholMaxRhs);  // one buffer serves both arenas
  if (s.schur_sn >= 0) {
    schur_tables(&s);
    s.work_bytes += 8 * (int64_t)(s.schur_ptr.size() + s.schur_src.size() + s.schur_dst.size() + s.schur_vptr.size() +
                                  s.schur_vsrc.size()) + 4 * (int64_t)s.schur_vld.size();
  }
  // launch tables
  s.chunk_ptr.assign((size_t)s.nlev + 1, 0);
  s.chunk_sn.clear();
  s.chunk_c0.clear();
  s.step_ptr.assign((size_t)s.nlev + 1, 0);
  s.step_nact.clear();
  s.step_tab.clear();
  s.tab.clear();
  for (int l = 0; l < s.nlev; l++) {
    for (int q = s.lev_ptr[l]; q < s.lev_ptr[l + 1]; q++) {
      const int J = s.lev_sn[q], sz = s.sn_first[J + 1] - s.sn_first[J], m = sz + s.sn_b[J];
      const bool kids = s.child_ptr[J + 1] > s.child_ptr[J];
      for (int c0 = 0; c0 < m; c0 += kCholChunk) {
        if (!kids && c0 + kCholChunk <= sz) continue;  // nothing to zero, nothing to gather
        s.chunk_sn.push_back(J);
        s.chunk_c0.push_back(c0);
      }
    }
    s.chunk_ptr[l + 1] = (int)s.chunk_sn.size();
    const int b0 = s.lev_ptr[l] + s.lev_nsmall[l], nbig = s.lev_ptr[l + 1] - b0;
    const int steps = nbig > 0 ? nblk_of(s.lev_sn[b0]) : 0;
    for (int kb = 0; kb < steps; kb++) {
      int nact = 0;
      while (nact < nbig && nblk_of(s.lev_sn[b0 + nact]) > kb) nact++;
      s.step_nact.push_back(nact);
      s.step_tab.push_back((int)s.tab.size());
      int64_t run = 0;
      s.tab.push_back(0);
      for (int a = 0; a < nact; a++) {
        const int J = s.lev_sn[b0 + a], sz = s.sn_first[J + 1] - s.sn_first[J], m = sz + s.sn_b[J];
        run += chol_row_tiles(sz, m, kb);
        if (run > 2000000000LL) {
          set_error("sparse Cholesky: a level has more than 2e9 row tiles");
          return PO_ERR_ARG;
        }
        s.tab.push_back((int)run);
      }
    }
    s.step_ptr[l + 1] = (int)s.step_nact.size();
  }
  return chol_scatter_table(s, n, colp, rows, &s.asm_ptr, &s.asm_dst, &s.asm_src);
}

const char *chol_form_name(int form) {
  static const char *const names[CHF_COUNT + CHF_SCHUR_COUNT] = {
      "assemble", "small", "blocked", "pack_factor", "fwd", "bwd", "pack_fwd", "pack_bwd", "schur_gather", "schur_fwd"};
  return form >= 0 && form < CHF_COUNT + CHF_SCHUR_COUNT ? names[form] : "";
}

void chol_kernel_forms(const CholSymbolic &s, int nv, int counts[CHF_COUNT]) {
  for (int f = 0; f < CHF_COUNT; f++) counts[f] = 0;
  const int slabs = (nv + kCholMaxRhs - 1) / kCholMaxRhs;
  for (int l = 0; l < s.nlev; l++) {
    const CholLevelPlan p = chol_level_plan(s, l);
    counts[CHF_ASSEMBLE] += p.nchunk > 0;
    counts[CHF_SMALL] += p.nsmall > 0;
    counts[CHF_BLOCKED] += p.nsteps > 0;
    counts[CHF_PACK_FACTOR] += p.ngroup > 0;
    counts[CHF_FWD] += slabs * (p.nfront > 0);
    counts[CHF_BWD] += slabs * (p.nfront > 0);
    counts[CHF_PACK_FWD] += slabs * (p.ngroup > 0);
    counts[CHF_PACK_BWD] += slabs * (p.ngroup > 0);
  }
}

void chol_schur_forms(const CholSymbolic &s, int nv, int counts[CHF_SCHUR_COUNT]) {
  for (int f = 0; f < CHF_SCHUR_COUNT; f++) counts[f] = 0;
  const int slabs = (nv + kCholMaxRhs - 1) / kCholMaxRhs;
  for (int l = 0; l < s.nlev; l++) {
    const CholLevelPlan p = chol_level_plan(s, l);
    counts[CHF_SCHUR_GATHER] += p.nschur;
    counts[CHF_SCHUR_FWD] += slabs * p.nschur;
  }
}

void chol_packing(const CholSymbolic &s, int64_t info[4], const int **group_first, const int **group_root,
                  const int **group_level, const int **front_order, const int64_t **upd_off) {
  info[0] = kCholTiny;
  info[1] = s.pack_cap;
  info[2] = (int64_t)s.grp_root.size();
  info[3] = chol_factor_levels(s);
  if (group_first) *group_first = s.grp_first.data();
  if (group_root) *group_root = s.grp_root.data();
  if (group_level) *group_level = s.grp_level.data();
  if (front_order) *front_order = s.front_order.data();
  if (upd_off) *upd_off = s.upd_off.data();
}

int chol_schur_solve_launches(const CholSymbolic &s) {
  const auto none = [](int, int) {};
  return chol_schur_panels(s.ns, s.schur_w, true, none, none) + chol_schur_panels(s.ns, s.schur_w, false, none, none);
}

int chol_factor_levels(const CholSymbolic &s) {
  int count = 0;
  for (int l = 0; l < s.nlev; l++) {
    const CholLevelPlan p = chol_level_plan(s, l);
    count += p.nchunk + p.nsmall + p.nsteps + p.ngroup + p.nschur > 0;
  }
  return count;
}

}  // namespace po
