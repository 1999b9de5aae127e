// Bond tables and the storage layouts built on them: site tensors (left / right kind), the two-site theta, the H
// environments and the overlap environments.  Host C++ (no HIP).
// NOT a translation unit of its own: #included by htn_plan.cpp (one unit, see its head); never name it on a build line.
#include "htn_core.h"

namespace htn {

// ---- bonds ---------------------------------------------------------------------------------------------------------
Bond::Bond(std::vector<std::pair<Sec, int>> items) {
    std::sort(items.begin(), items.end(), [](const std::pair<Sec, int>& a, const std::pair<Sec, int>& b) { return a.first < b.first; });
    for (auto& it : items) {
        if (it.second <= 0) continue;
        index[skey(it.first)] = (int)secs.size();
        secs.push_back(it.first);
        dims.push_back(it.second);
        int32_t rec[3] = {it.first.N, it.first.j, it.second};
        key.append((const char*)rec, sizeof(rec));
        seckey.append((const char*)rec, 2 * sizeof(int32_t));
    }
}
int64_t Bond::dim_full(const Sym& sym) const {
    int64_t d = 0;
    for (size_t i = 0; i < secs.size(); ++i) d += (int64_t)sym.qdim(secs[i]) * dims[i];
    return d;
}
int Bond::multiplets() const {
    int d = 0;
    for (int v : dims) d += v;
    return d;
}

// ---- layouts -------------------------------------------------------------------------------------------------------
SiteLayoutP build_site_layout(const Sym& sym, char kind, BondP bl, BondP br) {
    auto lay = std::make_shared<SiteLayout>();
    lay->kind = kind;
    lay->bl = bl;
    lay->br = br;
    int64_t off = 0;
    std::vector<Sec> tmp;
    auto add_block = [&](Sec l, int s, Sec r, BlockRec rec) {
        const Key k = mk(l.N, l.j, s, r.N, r.j);
        lay->bidx[k] = (int)lay->blocks.size();
        lay->bkeys.push_back(k);
        lay->blocks.push_back(rec);
    };
    if (kind == 'L') {
        for (size_t ri = 0; ri < br->secs.size(); ++ri) {
            const Sec r = br->secs[ri];
            std::vector<Grp> groups;
            for (int s = 0; s < sym.n_site; ++s) {
                sym.split(r, s, tmp);
                for (Sec l : tmp)
                    if (bl->has(l)) groups.push_back({l, s});
            }
            std::sort(groups.begin(), groups.end(), [](const Grp& a, const Grp& b) { return a.sec < b.sec || (a.sec == b.sec && a.s < b.s); });
            int rows = 0;
            for (auto& g : groups) rows += bl->dim(g.sec);
            if (rows == 0) continue;
            const int n = br->dims[ri];
            int ro = 0;
            for (auto& g : groups) {
                add_block(g.sec, g.s, r, {off + ro, bl->dim(g.sec), n, rows});
                ro += bl->dim(g.sec);
            }
            lay->midx[skey(r)] = (int)lay->mats.size();
            lay->mats.push_back({r, off, rows, n, groups});
            off += (int64_t)rows * n;
        }
    } else {
        for (size_t li = 0; li < bl->secs.size(); ++li) {
            const Sec l = bl->secs[li];
            std::vector<Grp> groups;
            for (int s = 0; s < sym.n_site; ++s) {
                sym.fuse(l, s, tmp);
                for (Sec r : tmp)
                    if (br->has(r)) groups.push_back({r, s});
            }
            std::sort(groups.begin(), groups.end(), [](const Grp& a, const Grp& b) { return a.s < b.s || (a.s == b.s && a.sec < b.sec); });
            int cols = 0;
            for (auto& g : groups) cols += br->dim(g.sec);
            if (cols == 0) continue;
            const int m = bl->dims[li];
            int co = 0;
            for (auto& g : groups) {
                add_block(l, g.s, g.sec, {off + (int64_t)co * m, m, br->dim(g.sec), m});
                co += br->dim(g.sec);
            }
            lay->midx[skey(l)] = (int)lay->mats.size();
            lay->mats.push_back({l, off, m, cols, groups});
            off += (int64_t)m * cols;
        }
    }
    lay->size = off;
    return lay;
}

ThetaLayoutP build_theta_layout(const Sym& sym, BondP bl, BondP br) {
    auto lay = std::make_shared<ThetaLayout>();
    lay->bl = bl;
    lay->br = br;
    std::map<Sec, std::vector<Grp>> rg, cg;
    std::vector<Sec> tmp;
    for (Sec a : bl->secs)
        for (int s1 = 0; s1 < sym.n_site; ++s1) {
            sym.fuse(a, s1, tmp);
            for (Sec c : tmp) rg[c].push_back({a, s1});
        }
    for (Sec b : br->secs)
        for (int s2 = 0; s2 < sym.n_site; ++s2) {
            sym.split(b, s2, tmp);
            for (Sec c : tmp) cg[c].push_back({b, s2});
        }
    int64_t off = 0;
    for (auto& kv : rg) {
        const Sec c = kv.first;
        auto ic = cg.find(c);
        if (ic == cg.end()) continue;
        ThetaLayout::Mat M;
        M.c = c;
        M.rows_g = kv.second;
        M.cols_g = ic->second;
        std::sort(M.rows_g.begin(), M.rows_g.end(), [](const Grp& a, const Grp& b) { return a.sec < b.sec || (a.sec == b.sec && a.s < b.s); });
        std::sort(M.cols_g.begin(), M.cols_g.end(), [](const Grp& a, const Grp& b) { return a.s < b.s || (a.s == b.s && a.sec < b.sec); });
        M.roffs.push_back(0);
        for (auto& g : M.rows_g) M.roffs.push_back(M.roffs.back() + bl->dim(g.sec));
        M.coffs.push_back(0);
        for (auto& g : M.cols_g) M.coffs.push_back(M.coffs.back() + br->dim(g.sec));
        M.rows = M.roffs.back();
        M.cols = M.coffs.back();
        M.off = off;
        for (size_t i = 0; i < M.rows_g.size(); ++i)
            for (size_t j = 0; j < M.cols_g.size(); ++j) {
                const Sec a = M.rows_g[i].sec, b = M.cols_g[j].sec;
                const Key k = mk(a.N, a.j, M.rows_g[i].s, c.N, c.j, M.cols_g[j].s, b.N, b.j);
                lay->bidx[k] = (int)lay->blocks.size();
                lay->bkeys.push_back(k);
                lay->blocks.push_back({off + M.roffs[i] + (int64_t)M.coffs[j] * M.rows, bl->dim(a), br->dim(b), M.rows});
            }
        off += (int64_t)M.rows * M.cols;
        lay->midx[skey(c)] = (int)lay->mats.size();
        lay->mats.push_back(std::move(M));
    }
    lay->size = off;
    return lay;
}

EnvLayoutP build_env_layout(const Sym& sym, char side, BondP bond, const std::vector<Lvl>& levels) {
    auto lay = std::make_shared<EnvLayout>();
    lay->side = side;
    lay->bond = bond;
    lay->levels = levels;
    lay->ident = side == 'L' ? 0 : (int)levels.size() - 1;
    int64_t off = 0;
    for (int w = 0; w < (int)levels.size(); ++w) {
        if (w == lay->ident) continue;
        for (size_t ki = 0; ki < bond->secs.size(); ++ki) {
            const Sec ket = bond->secs[ki];
            for (size_t bi = 0; bi < bond->secs.size(); ++bi) {
                const Sec bra = bond->secs[bi];
                if (!sym.connects(ket, levels[w].dN, levels[w].k, bra)) continue;
                Key k;
                EnvLayout::Blk rec;
                if (side == 'L') {
                    k = mk(bra.N, bra.j, w, ket.N, ket.j);
                    rec = {off, bond->dims[bi], bond->dims[ki]};
                } else {
                    k = mk(ket.N, ket.j, w, bra.N, bra.j);
                    rec = {off, bond->dims[ki], bond->dims[bi]};
                }
                lay->bidx[k] = (int)lay->blocks.size();
                lay->bkeys.push_back(k);
                lay->blocks.push_back(rec);
                lay->by_ket[mk(w, ket.N, ket.j)].push_back(bra);
                off += (int64_t)bond->dims[bi] * bond->dims[ki];
            }
        }
    }
    lay->size = off;
    return lay;
}

// ---- overlap environments of orthogonalised DMRG (htn_core.h: OvlLayout) --------------------------------------------------
OvlLayoutP build_ovl_layout(BondP rows, BondP cols) {
    auto o = std::make_shared<OvlLayout>();
    o->rows = rows;
    o->cols = cols;
    for (size_t q = 0; q < rows->secs.size(); ++q) {
        const Sec c = rows->secs[q];
        const int nc = cols->dim(c);
        if (nc <= 0) continue;
        o->index[skey(c)] = (int)o->secs.size();
        o->secs.push_back(c);
        o->off.push_back(o->size);
        o->m.push_back(rows->dims[q]);
        o->n.push_back(nc);
        o->size += (int64_t)rows->dims[q] * nc;
    }
    return o;
}

}  // namespace htn
