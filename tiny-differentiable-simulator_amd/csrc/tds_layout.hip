// tds_layout.hip — host side of the general step kernel that no kernel build needs: the padded dof count and the
// per-environment LDS layout (TdsLds).  Compiled once; the constants it shares with the kernel are in tds_kernels.h.
#include <string.h>

#include "tds_device_model.h"
#include "tds_kernels.h"

// padded dof count = template parameter NDP of the kernel.  Besides the coarse widths (8/16/24/32) the
// widths of the two benchmark robots are instantiated exactly for their natural lane count
// (Ant: 14 dof on 16 lanes, Laikago: 18 dof on 32 lanes): LDL^T and the row solves scale with NDP^2.
int tds_padded_dof(int nd, int lanes) {
  if (lanes == 16 && nd > 8 && nd <= 14) return 14;
  if (lanes == 32 && nd > 16 && nd <= 18) return 18;
  return nd <= 8 ? 8 : (nd <= 16 ? 16 : (nd <= 24 ? 24 : 32));
}

template <typename T>
TdsLds tds_make_lds_layout(const DevModel<T> &m, int na_cap, int lanes_per_env, bool w2) {
  TdsLds L;
  memset(&L, 0, sizeof(L));
  const int nl = m.num_links;
  const int ndp = tds_padded_dof(m.dof_qd, lanes_per_env);
  L.NLp = nl;
  L.NDP = ndp;
  L.NDs = ndp + 1;  // odd row stride: lane == row accesses hit distinct LDS banks
  const int ncp = m.has_plane ? m.num_cp : 0;
  L.NCPp = ncp > 0 ? ncp : 1;
  // two-body worlds: the contacts between the bodies are a second pass through the same row store
  const int npc = m.num_bodies >= 2 ? m.num_pc : 0;
  L.NPCp = npc > 0 ? npc : 1;
  const int nct = ncp > npc ? ncp : npc;  // contacts of the larger pass
  if (na_cap <= 0 || na_cap > nct) na_cap = nct;
  L.zrows = 3 * na_cap;            // constraint rows kept in LDS
  L.ovrows = 3 * nct - L.zrows;    // surplus rows per environment (global scratch slab)
  int o = 0;
  // persistent for the whole step
  L.xrec = o; o += m.input_dim + 4 + (w2 ? 4 : 0);  // + x_{t-1}, the done flag, the reward and the "records are out" flag of
                                                    //   the step loop (two-wavefront layout: + 2 .. + 5 are the contact counts
                                                    //   and flags handed between the wavefronts)
  // two pairs with disjoint lifetimes share their storage:
  //   swd  (world motion axes per dof: phases C..J)  |  rows (b, 1/(G+cfm), G per constraint row: K..L)
  //   cp   (contact points: phases I..K)             |  xrow (impulses x of all rows: L)
  {
    const int a = 6 * L.NDs, b = 3 * L.zrows;
    if (npc > 0) {  // (the second contact pass builds its rows from the motion axes after the first one's row scalars)
      L.swd = o; o += a;
      L.rows = o; o += b;
    } else {
      L.swd = o; L.rows = o; o += a > b ? a : b;
    }
  }
  {
    const int a = ncp ? 5 * L.NCPp : 0, b = 3 * nct;
    L.cp = o; L.xrow = o; o += a > b ? a : b;
  }
  L.pc = o;
  if (npc > 0) o += 17 * L.NPCp;  // contact list of the pairs: lives from the narrowphase to the second pass
  L.Lp = o;   o += (ndp * (ndp - 1)) / 2;
  L.Lh = o;   // two-wavefront pipeline (narrow kernels): row-major copy of the first ndp/2 columns of L, 16 + 1 rows
  if (w2 && ndp <= 16) o += 17 * (ndp / 2);  // (+ one row for the lanes of wider groups that own no row)
  L.dinv = o; o += (w2 ? 4 : 3) * ndp;  // 1/D | sqrt(1/D) | column scratch of the wide LDL^T / rhs exchange (| y~)
  L.tau = o;
  if (tds_parks_tau(ndp, w2)) o += nl;  // (the generalised forces wait here from the PD block to phase F)
  // three phase groups share one region:
  //   1. kinematics sweep:   per-link records [X_world(12) | v(6)]              stride TDS_S1
  //   2. composite sweep:    per-link records [f or F(6) | Ic(10)] stride TDS_S2
  //   3. constraint rows:    Z[zrows][NDs]
  const int u = o;
  int g1 = u;
  L.Xw = g1; g1 += TDS_S1 * L.NLp;
  L.v = g1; g1 += TDS_S1 * m.num_lc_slots;
  // (two-wavefront workgroups: the helper wavefront reads X_world and writes the rows while the main one sweeps the
  //  inertias — the three groups are laid out one after the other)
  int g2 = w2 ? g1 : u;
  L.IA = g2; L.pA = g2; L.F = g2; L.Ic = g2 + 6; L.a = g2; g2 += TDS_S2 * L.NLp;
  int g3 = w2 ? g2 : u;
  L.Z = g3; g3 += L.zrows * L.NDs;
  // Gram form of the contact solve (tds_gram_solve): its 16 x 17 buffer + 16 zeros reuse the two sweep groups
  // Opt-in (TDS_HIP_GRAM=1): measured 0.4k of 32k cycles better than the z~ sweep at Ant x 4096 (profiles/r02d_gram_mfma.txt),
  // and an environment's low-order bits then depend on whether its wavefront-mates push NA past 5 (sweep) or not (Gram).
  L.gram_ok = (tds_opt_now_flag(TDS_OPT_GRAM) && w2 && lanes_per_env == 16 && ndp <= 16 && m.num_bodies < 2 &&
               L.Z - L.Xw >= TDS_GRAM_ZEROS + 16) ? 1 : 0;
  o = g1 > g2 ? g1 : g2;
  o = o > g3 ? o : g3;
  o = (o + 1) & ~1;  // keep 16-byte alignment of every env region for T = double
  L.stride = o;
  L.in_dim = m.input_dim;
  L.adim = m.action_dim;
  L.nqnd = m.dof_q + m.dof_qd;
  return L;
}

template TdsLds tds_make_lds_layout<double>(const DevModel<double> &, int, int, bool);
template TdsLds tds_make_lds_layout<float>(const DevModel<float> &, int, int, bool);
