// ik_golden.cpp — runs the reference's TinyInverseKinematics::compute on cases read from stdin and prints its answers,
// for tools/ik_golden.py (which draws the cases and writes tests/golden/ik_reference.npz).  It includes the reference's
// headers by -I path and is built by hand (tools/README.md); the binary is not committed.
//
// A case, whitespace separated:
//   urdf floating method K max_iterations lambda target_tol step_tol alpha weight_ref have_ref nq
//   q_init[nq]  (q_ref[nq] if have_ref)  K x (link  body_point[3]  target[3])
// The answer, one line (the reference's loader prints lines of its own):
//   IK status iterations residual q[nq] margins_ok rank_ok
// margins_ok: at every iteration the residual differs from target_tol and sum delta^2 from step_tol^2 by more than
// 1e-6 relative.  rank_ok: at every iteration every singular value of J is above 1e-6 or below 1e-12 of the largest.
// Both are found by running compute again with max_iterations = 1, 2, ...: run i ends with the q after i iterations and
// the residual of iteration i - 1.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include <Eigen/SVD>

#include "math/tiny/tiny_algebra.hpp"
#include "math/tiny/tiny_double_utils.h"
#include "tiny_inverse_kinematics.h"
#include "urdf/urdf_cache.hpp"
#include "world.hpp"

typedef TinyAlgebra<double, TINY::DoubleUtils> Alg;
typedef Alg::VectorX VecX;

struct Case {
  int method, K, max_it, have_ref, nq;
  double lambda, ttol, stol, alpha, wref;
  std::vector<double> q_init, q_ref;
  std::vector<int> links;
  std::vector<double> bp, tgt;
};

static bool far_from(double v, double bound) { return std::fabs(v - bound) > 1e-6 * bound; }

// the stacked Jacobian as compute builds it (tiny_inverse_kinematics.h:162-186), for its singular values only
static bool rank_gap(const tds::MultiBody<Alg> &mb, const Case &c, const VecX &q) {
  tds::Transform<Alg> bw;
  std::vector<tds::Transform<Alg>> lw, lb;
  tds::forward_kinematics_q<Alg>(mb, q, &bw, &lw, &lb);
  const int nd = mb.dof_qd();
  Eigen::MatrixXd J = Eigen::MatrixXd::Zero(3 * c.K, nd);
  for (int k = 0; k < c.K; ++k) {
    Alg::Vector3 p = lb[c.links[k]].apply(Alg::Vector3(c.bp[3 * k], c.bp[3 * k + 1], c.bp[3 * k + 2]));
    auto G = tds::point_jacobian<Alg>(mb, q, c.links[k], p, true);
    for (int i = 0; i < 3; ++i)
      for (int j = mb.is_floating() ? 6 : 0; j < nd; ++j) J(3 * k + i, j) = G(i, j);
  }
  Eigen::JacobiSVD<Eigen::MatrixXd> svd(J);
  const auto &sv = svd.singularValues();
  for (int i = 0; i < sv.size(); ++i)
    if (sv(0) > 0 && sv(i) <= 1e-6 * sv(0) && sv(i) >= 1e-12 * sv(0)) return false;
  return true;
}

template <TINY::TinyIKMethod Method>
static void run(const tds::MultiBody<Alg> &mb, const Case &c) {
  TINY::TinyInverseKinematics<Alg, Method> ik;
  for (int k = 0; k < c.K; ++k) {
    TINY::TinyIKTarget<Alg> t(c.links[k], Alg::Vector3(c.tgt[3 * k], c.tgt[3 * k + 1], c.tgt[3 * k + 2]));
    t.body_point = Alg::Vector3(c.bp[3 * k], c.bp[3 * k + 1], c.bp[3 * k + 2]);
    ik.targets.push_back(t);
  }
  ik.lambda = c.lambda, ik.target_tolerance = c.ttol, ik.step_tolerance = c.stol, ik.alpha = c.alpha;
  ik.weight_reference = c.wref;
  VecX q0(c.nq), q(c.nq), prev(c.nq);
  for (int i = 0; i < c.nq; ++i) q0[i] = c.q_init[i];
  if (c.have_ref) {
    ik.q_reference = VecX(c.nq);
    for (int i = 0; i < c.nq; ++i) ik.q_reference[i] = c.q_ref[i];
  }
  bool margins = true, rank = true;
  const int qo = mb.is_floating() ? 7 : 0;
  prev = q0;
  for (int n = 1; n <= c.max_it; ++n) {
    ik.max_iterations = n;
    auto r = ik.compute(mb, q0, q);
    if (Method == TINY::IK_JAC_PINV) rank = rank && rank_gap(mb, c, prev);
    margins = margins && far_from(r.residual, c.ttol);
    if (r.ik_status == TINY::IK_RESULT_REACHED) break;
    double sq = 0;
    for (int i = qo; i < c.nq; ++i) {
      const double moved = c.have_ref ? (q[i] - c.wref * c.q_ref[i]) / (1 - c.wref) : q[i];
      const double d = (moved - prev[i]) / c.alpha;
      sq += d * d;
    }
    margins = margins && far_from(sq, c.stol * c.stol);
    if (r.ik_status != TINY::IK_RESULT_FAILED) break;
    prev = q;
  }
  ik.max_iterations = c.max_it;
  auto r = ik.compute(mb, q0, q);
  printf("IK %d %d %.17g", (int)r.ik_status, r.iter, r.residual);
  for (int i = 0; i < c.nq; ++i) printf(" %.17g", q[i]);
  printf(" %d %d\n", margins ? 1 : 0, rank ? 1 : 0);
}

int main(int argc, char **argv) {
  if (argc < 2) return fprintf(stderr, "usage: ik_golden <reference root> < cases\n"), 2;
  const std::string root = argv[1];
  tds::World<Alg> world;
  tds::UrdfCache<Alg> cache;
  std::map<std::string, tds::MultiBody<Alg> *> bodies;
  std::string file;
  int floating;
  while (std::cin >> file >> floating) {
    Case c;
    std::cin >> c.method >> c.K >> c.max_it >> c.lambda >> c.ttol >> c.stol >> c.alpha >> c.wref >> c.have_ref >> c.nq;
    c.q_init.resize(c.nq);
    for (double &v : c.q_init) std::cin >> v;
    if (c.have_ref) {
      c.q_ref.resize(c.nq);
      for (double &v : c.q_ref) std::cin >> v;
    }
    c.links.resize(c.K), c.bp.resize(3 * c.K), c.tgt.resize(3 * c.K);
    for (int k = 0; k < c.K; ++k) {
      std::cin >> c.links[k];
      for (int i = 0; i < 3; ++i) std::cin >> c.bp[3 * k + i];
      for (int i = 0; i < 3; ++i) std::cin >> c.tgt[3 * k + i];
    }
    const std::string key = file + (floating ? "+floating" : "");
    if (!bodies.count(key)) {
      bodies[key] = cache.construct(root + "/data/" + file, world, false, floating != 0);
      bodies[key]->base_X_world().set_identity();
    }
    const tds::MultiBody<Alg> &mb = *bodies[key];
    if (mb.dof() != c.nq) return fprintf(stderr, "%s: dof %d, case has %d\n", key.c_str(), mb.dof(), c.nq), 1;
    if (c.method == 0)
      run<TINY::IK_JAC_TRANSPOSE>(mb, c);
    else if (c.method == 1)
      run<TINY::IK_JAC_PINV>(mb, c);
    else
      run<TINY::IK_DAMPED_LM>(mb, c);
  }
  return 0;
}
