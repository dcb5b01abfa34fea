// sharded.hip -- the multi-GPU part of the C ABI (include/nbody_hip_comm.h): communicators (RCCL over xGMI, or
// direct peer copies when one process drives all devices) and the sharded Direct N^2 system of BASELINE config 3.
// The reference is single-GPU; what this spreads over the ranks is launchDirectForceKernel
// (src/cuda/force_direct.cu:88-98) and the step of Integrator::integrate (src/cuda/integrator.cu:224-238).
//
// Everything here is host orchestration over the entry points of nbody_hip.h plus one small kernel (sum of the
// received reaction blocks fused with the kick).  One host thread issues the work of all local ranks PHASE BY
// PHASE; every cross-rank dependency is a HIP event recorded in an earlier phase, so there is no circular wait.
//
//   phase        compute stream of rank r                         comm stream of rank r
//   drift        x += v dt + a dt^2/2 (own rows of posm_all)
//                record ev_ready
//   gather                                                        wait ev_ready ; P2P: wait ev_read of every peer
//                                                                 (its kernels of the last step still read its
//                                                                 posm_all), push own rows into every peer's
//                                                                 posm_all ; RCCL: in-place ncclAllGather
//                                                                 record ev_gather
//   own x own    symmetric kernel -> mine        (overlaps the gather)
//   pairs        wait ev_gather (P2P: of every rank) ; per task: two-set kernel, action added to mine,
//                reaction -> the task's send block ; record ev_read
//   exchange                                                      wait ev_read ; P2P: copy each send block into
//                                                                 the owner's receive block ; RCCL: grouped
//                                                                 ncclSend / ncclRecv ; record ev_sent
//   finalize     wait ev_sent (P2P: of every sender) ; a_new = mine + received blocks in rank-distance order ;
//                v += (a_old + a_new) dt / 2
// WAR hazards: a receive block is rewritten by a sender only after the sender passed "pairs" of the new step, i.e.
// after it saw the owner's ev_gather of the new step, which the owner records after its own finalize of the old one.
//
// The five events of a rank x, (1) in a force phase and (2) in compute_forces around it (upload, read-back):
//
//   event      recorded on               waited on by                                what the wait protects
//   ev_ready 1 x.compute, after drift    x.comm                                      the gather reads x's own rows as drifted
//            2 r0.compute, after pack    nobody (the record after the force phase replaces it)
//            2 x.compute, after finalize x.comm                                      the read-back gathers acc[cur] as finalized
//   ev_gather 1 x.comm, after gather     RCCL: x.compute; P2P: p.compute, p != x     the pair kernels read posm_all complete
//            2 r0.compute, after the     p.compute, p != r0                          p's kernels read the uploaded posm_all
//              copies into the peers
//   ev_read  1 x.compute, after the      x.comm                                      the exchange sends the blocks as written
//              cross-shard kernels       P2P, next gather: p.comm, p != x            x.posm_all is overwritten after x read it
//            2 (that same record)        r0.compute, before the upload               the same, for the upload's copies
//   ev_sent  1 x.comm, after exchange    RCCL: x.compute; P2P: the compute streams   the finalize sums blocks that have arrived
//                                        of the ranks x sends to
//            2 x.comm, after read-back   r0.compute                                  unpack3 reads r0.stage complete
//   ev_aux   2 null stream of r0, entry  r0.compute                                  the caller's work on d precedes the pack
//            2 r0.compute, at the end    null stream of r0                           the caller's next work sees d->acc_*
//
// The RCCL gather needs no ev_read: every rank's posm_all is written by its OWN comm stream, behind its own ev_ready.

#include <cstring>
#include <vector>

#include "comm.h"
#include "shard_plan.h"

namespace nbh {

// ---- RCCL, resolved at run time -----------------------------------------------------------------------------------
Rccl* rccl_load() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r.so ? &r : nullptr;
  tried = true;
  // the copy already mapped into the process (PyTorch ships one with the same soname) wins; then the loader path
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* so = dlopen(names[0], RTLD_NOW | RTLD_NOLOAD);
  for (int k = 0; !so && k < 3; k++) so = dlopen(names[k], RTLD_NOW | RTLD_LOCAL);
  if (!so) return nullptr;
  bool ok = true;
#define NBH_SYM(field, name)                                              \
  r.field = reinterpret_cast<decltype(r.field)>(dlsym(so, name));         \
  ok = ok && r.field != nullptr
  NBH_SYM(GetUniqueId, "ncclGetUniqueId");
  NBH_SYM(CommInitRank, "ncclCommInitRank");
  NBH_SYM(CommInitAll, "ncclCommInitAll");
  NBH_SYM(CommDestroy, "ncclCommDestroy");
  NBH_SYM(AllGather, "ncclAllGather");
  NBH_SYM(AllReduce, "ncclAllReduce");
  NBH_SYM(Send, "ncclSend");
  NBH_SYM(Recv, "ncclRecv");
  NBH_SYM(GroupStart, "ncclGroupStart");
  NBH_SYM(GroupEnd, "ncclGroupEnd");
  NBH_SYM(GetErrorString, "ncclGetErrorString");
#undef NBH_SYM
  if (!ok) {
    dlclose(so);
    return nullptr;
  }
  r.so = so;
  return &r;
}

static_assert(sizeof(nbody_hip_comm_id) == sizeof(ncclUniqueId), "nbody_hip_comm_id must hold an ncclUniqueId");
static_assert(kShardMaxRanks == NBODY_HIP_MAX_RANKS, "shard_plan.h is checked for the world sizes the ABI accepts");

// a_new = mine + the received reaction blocks (fixed order) ; optional kick
struct InBlocks {
  int n;
  const float4* buf[NBODY_HIP_MAX_RANKS / 2];
  unsigned int j0[NBODY_HIP_MAX_RANKS / 2], j1[NBODY_HIP_MAX_RANKS / 2];
};
__global__ __launch_bounds__(kBlock) void shard_finalize_kernel(const float4* __restrict__ mine, InBlocks in, int n,
                                                                float4* __restrict__ acc_new,
                                                                float4* __restrict__ vel,
                                                                const float4* __restrict__ acc_old, float half_dt,
                                                                int kick) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float4 a = mine[i];
  for (int k = 0; k < in.n; k++) {
    if ((unsigned)i >= in.j0[k] && (unsigned)i < in.j1[k]) {
      const float4 b = in.buf[k][(unsigned)i - in.j0[k]];
      a.x += b.x; a.y += b.y; a.z += b.z;
    }
  }
  a.w = 0.f;
  acc_new[i] = a;
  if (kick) {
    float4 v = vel[i];
    const float4 o = acc_old[i];
    v.x = kick1(v.x, o.x, a.x, half_dt);
    v.y = kick1(v.y, o.y, a.y, half_dt);
    v.z = kick1(v.z, o.z, a.z, half_dt);
    vel[i] = v;
  }
}

}  // namespace nbh

using namespace nbh;

// ---- communicators ------------------------------------------------------------------------------------------------
extern "C" int nbody_hip_shard_bounds(size_t n, int world, int rank, size_t* shard, size_t* lo, size_t* hi) {
  if (world < 1 || rank < 0 || rank >= world) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "rank %d outside world %d", rank, world);
  const ShardBounds b = shard_bounds(n, world, rank);
  if (shard) *shard = b.shard;
  if (lo) *lo = b.lo;
  if (hi) *hi = b.hi;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_pair_schedule(int world, int rank, size_t S, size_t rows[][5], int max_rows) {
  if (world < 1 || rank < 0 || rank >= world) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "rank %d outside world %d", rank, world);
  int at = 0;
  const int k = pair_schedule(world, rank, S, [&](size_t i0, size_t i1, int sh, size_t j0, size_t j1) {
    if (rows && at < max_rows) {
      rows[at][0] = i0; rows[at][1] = i1; rows[at][2] = (size_t)sh; rows[at][3] = j0; rows[at][4] = j1;
    }
    at++;
  });
  if (rows && k > max_rows) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "schedule has %d rows, room for %d", k, max_rows);
  return k;
}

extern "C" int nbody_hip_comm_init_all(int ndev, const int* devices, int transport, nbody_hip_comm** out) {
  nbh::DeviceGuard dev_guard;  // the caller's current device is restored on return
  if (!out) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  *out = nullptr;
  if (ndev < 1 || ndev > NBODY_HIP_MAX_RANKS)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "ndev must be in [1, %d]", NBODY_HIP_MAX_RANKS);
  if (transport != NBODY_HIP_TRANSPORT_P2P && transport != NBODY_HIP_TRANSPORT_RCCL)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "unknown transport %d", transport);
  const int have = nbody_hip_device_count();
  if (have <= 0) return NBH_FAIL(NBODY_HIP_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  std::vector<int> dev(ndev);
  for (int r = 0; r < ndev; r++) {
    dev[r] = devices ? devices[r] : r;
    if (dev[r] < 0 || dev[r] >= have)
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "device %d of rank %d out of range [0,%d)", dev[r], r, have);
    if (transport == NBODY_HIP_TRANSPORT_RCCL)
      for (int q = 0; q < r; q++)
        if (dev[q] == dev[r]) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "RCCL needs distinct devices (device %d twice)", dev[r]);
  }
  // peer access between distinct devices (both transports copy between local ranks)
  for (int r = 0; r < ndev; r++)
    for (int q = 0; q < ndev; q++) {
      if (dev[r] == dev[q]) continue;
      NBH_HIP(hipSetDevice(dev[r]));
      int can = 0;
      NBH_HIP(hipDeviceCanAccessPeer(&can, dev[r], dev[q]));
      if (!can) return NBH_FAIL(NBODY_HIP_ERR_DEVICE, "device %d cannot access device %d", dev[r], dev[q]);
      const hipError_t e = hipDeviceEnablePeerAccess(dev[q], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
        return NBH_FAIL(NBODY_HIP_ERR_DEVICE, "hipDeviceEnablePeerAccess(%d -> %d): %s", dev[r], dev[q], hipGetErrorString(e));
      (void)hipGetLastError();
    }
  nbody_hip_comm* c = new nbody_hip_comm();
  c->world = ndev;
  c->transport = transport;
  c->local.resize(ndev);
  for (int r = 0; r < ndev; r++) {
    c->local[r].rank = r;
    c->local[r].device = dev[r];
  }
  if (transport == NBODY_HIP_TRANSPORT_RCCL) {
    Rccl* api = rccl_load();
    if (!api) {
      delete c;
      return NBH_FAIL((nbody_hip_status)NBODY_HIP_ERR_COMM, "librccl.so.1 cannot be loaded: %s", dlerror());
    }
    std::vector<ncclComm_t> comms(ndev);
    const ncclResult_t r_ = api->CommInitAll(comms.data(), ndev, dev.data());
    if (r_ != ncclSuccess) {
      delete c;
      return NBH_FAIL((nbody_hip_status)NBODY_HIP_ERR_COMM, "ncclCommInitAll: %s", api->GetErrorString(r_));
    }
    for (int r = 0; r < ndev; r++) c->local[r].nccl = comms[r];
  }
  *out = c;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_comm_unique_id(nbody_hip_comm_id* id) {
  if (!id) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null argument");
  Rccl* api = rccl_load();
  if (!api) return NBH_FAIL((nbody_hip_status)NBODY_HIP_ERR_COMM, "librccl.so.1 cannot be loaded: %s", dlerror());
  ncclUniqueId u;
  NBH_NCCL(api, api->GetUniqueId(&u));
  memcpy(id->bytes, &u, sizeof(u));
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_comm_init_rank(int device, int rank, int world, const nbody_hip_comm_id* id,
                                        nbody_hip_comm** out) {
  nbh::DeviceGuard dev_guard;  // the caller's current device is restored on return
  if (!out || !id) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null argument");
  *out = nullptr;
  if (world < 1 || world > NBODY_HIP_MAX_RANKS || rank < 0 || rank >= world)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "rank %d / world %d out of range (at most %d ranks)", rank, world, NBODY_HIP_MAX_RANKS);
  const int have = nbody_hip_device_count();
  if (have <= 0) return NBH_FAIL(NBODY_HIP_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= have) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "device %d out of range [0,%d)", device, have);
  Rccl* api = rccl_load();
  if (!api) return NBH_FAIL((nbody_hip_status)NBODY_HIP_ERR_COMM, "librccl.so.1 cannot be loaded: %s", dlerror());
  NBH_HIP(hipSetDevice(device));
  ncclUniqueId u;
  memcpy(&u, id->bytes, sizeof(u));
  ncclComm_t comm = nullptr;
  NBH_NCCL(api, api->CommInitRank(&comm, world, u, rank));
  nbody_hip_comm* c = new nbody_hip_comm();
  c->world = world;
  c->transport = NBODY_HIP_TRANSPORT_RCCL;
  c->local.resize(1);
  c->local[0].rank = rank;
  c->local[0].device = device;
  c->local[0].nccl = comm;
  *out = c;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_comm_info(const nbody_hip_comm* c, int* world, int* nlocal, int* transport,
                                   int local_ranks[NBODY_HIP_MAX_RANKS]) {
  if (!c) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null communicator");
  if (world) *world = c->world;
  if (nlocal) *nlocal = (int)c->local.size();
  if (transport) *transport = c->transport;
  if (local_ranks)
    for (size_t k = 0; k < c->local.size(); k++) local_ranks[k] = c->local[k].rank;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_comm_destroy(nbody_hip_comm* c) {
  nbh::DeviceGuard dev_guard;  // the caller's current device is restored on return
  if (!c) return NBODY_HIP_OK;
  NBH_DESTROY_BEGIN
  if (c->transport == NBODY_HIP_TRANSPORT_RCCL) {
    Rccl* api = rccl_load();
    for (auto& m : c->local)
      if (m.nccl && api) {
        (void)hipSetDevice(m.device);
        (void)api->CommDestroy(m.nccl);
      }
  }
  delete c;
  NBH_DESTROY_END
}

// ---- the sharded Direct system --------------------------------------------------------------------------------------
namespace {

struct Shard {
  int rank = 0, device = 0;
  nbody_hip_ctx* ctx = nullptr;
  hipStream_t compute = nullptr, comm = nullptr;
  ncclComm_t nccl = nullptr;
  float4 *posm_all = nullptr, *vel = nullptr, *acc[2] = {nullptr, nullptr}, *mine = nullptr, *stage = nullptr;
  double* esum = nullptr;  // 2 W doubles (energies of every rank, RCCL all-gather)
  // pair mode: this rank's entries of the plan; send[k] takes the reactions of tasks[k] (row 0 = body j0), recv[k] is the
  // block of incoming[k]; `in` is what the finalize kernel takes, complete once recv is allocated
  const ShardRankPlan* plan = nullptr;
  std::vector<float4*> send, recv;
  InBlocks in = {};
  hipEvent_t ev_ready = nullptr, ev_gather = nullptr, ev_read = nullptr, ev_sent = nullptr, ev_aux = nullptr;
  hipEvent_t t0 = nullptr, t1 = nullptr;
};

}  // namespace

struct nbody_hip_sharded_direct {
  nbody_hip_comm* comm = nullptr;
  size_t n = 0, S = 0;
  int W = 1;
  float G = 1.f, eps = 0.f, eps2 = 0.f;
  bool pair_mode = true;
  int cur = 0;  // acc[cur] holds the current accelerations on every shard
  bool have_state = false;
  ShardedDirectPlan plan;  // pair mode: the tasks and reaction blocks of all W ranks; otherwise W empty lists
  std::vector<Shard> sh;
  Shard* by_rank[NBODY_HIP_MAX_RANKS] = {};
  float4* own(Shard& s) const { return s.posm_all + (size_t)s.rank * S; }
};

// the shared opening of the entry points: the caller's current device is restored on return
#define NBH_DIRECT_ENTER(s)    \
  nbh::DeviceGuard dev_guard;  \
  if (!(s)) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null system")
#define NBH_DIRECT_ENTER_WITH_STATE(s, message) \
  NBH_DIRECT_ENTER(s);                          \
  if (!(s)->have_state) return NBH_FAIL(NBODY_HIP_ERR_STATE, message)

static void shard_release(Shard& s) {
  (void)hipSetDevice(s.device);
  if (s.compute) (void)hipStreamSynchronize(s.compute);
  if (s.comm) (void)hipStreamSynchronize(s.comm);
  (void)hipFree(s.posm_all); (void)hipFree(s.vel); (void)hipFree(s.acc[0]); (void)hipFree(s.acc[1]);
  (void)hipFree(s.mine); (void)hipFree(s.stage); (void)hipFree(s.esum);
  for (float4* b : s.send) (void)hipFree(b);
  for (float4* b : s.recv) (void)hipFree(b);
  for (hipEvent_t e : {s.ev_ready, s.ev_gather, s.ev_read, s.ev_sent, s.ev_aux, s.t0, s.t1})
    if (e) (void)hipEventDestroy(e);
  if (s.ctx) (void)nbody_hip_ctx_destroy(s.ctx);
  if (s.compute) (void)hipStreamDestroy(s.compute);
  if (s.comm) (void)hipStreamDestroy(s.comm);
}

extern "C" int nbody_hip_sharded_direct_destroy(nbody_hip_sharded_direct* s) {
  nbh::DeviceGuard dev_guard;  // the caller's current device is restored on return
  if (!s) return NBODY_HIP_OK;
  NBH_DESTROY_BEGIN
  for (auto& x : s->sh) shard_release(x);
  delete s;
  NBH_DESTROY_END
}

extern "C" int nbody_hip_sharded_direct_create(nbody_hip_comm* comm, size_t n, float G, float eps,
                                               nbody_hip_sharded_direct** out) {
  nbh::DeviceGuard dev_guard;  // the caller's current device is restored on return
  if (!comm || !out) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null argument");
  *out = nullptr;
  if (n == 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count must be greater than 0");
  if (n > 100000000u) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count exceeds maximum supported (100M)");
  if (!(G > 0.0f) || !(G < INFINITY)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Gravitational constant must be positive and finite");
  if (!(eps >= 0.0f) || !(eps < INFINITY)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Softening parameter must be non-negative and finite");
  nbody_hip_sharded_direct* s = new nbody_hip_sharded_direct();
  s->comm = comm;
  s->n = n;
  s->W = comm->world;
  s->S = (n + (size_t)s->W - 1) / (size_t)s->W;
  s->G = G;
  s->eps = eps;
  s->eps2 = eps * eps;  // force_calculator.hpp:52-57
  s->pair_mode = direct_pairs_ok(s->eps2) && s->W > 1;
  const size_t S = s->S, all = S * (size_t)s->W;
  s->sh.resize(comm->local.size());
  auto fail = [&](int rc) {
    nbody_hip_sharded_direct_destroy(s);
    return rc;
  };
  // the plan's invariants, asserted once (shard_plan_check proves them for every world size the ABI accepts)
  int from = 0, to = 0;
  const PlanFault fault = s->pair_mode ? sharded_direct_plan(s->plan, s->W, S, &from, &to) : kPlanOk;
  if (fault == kPlanMismatch) return fail(NBH_FAIL(NBODY_HIP_ERR_STATE, "schedule mismatch between ranks %d and %d", from, to));
  if (fault == kPlanTooManyBlocks) return fail(NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "too many incoming blocks"));
  s->plan.rank.resize((size_t)s->W);  // (without pair mode: W empty lists)
  for (size_t k = 0; k < comm->local.size(); k++) {
    Shard& x = s->sh[k];
    x.rank = comm->local[k].rank;
    x.device = comm->local[k].device;
    x.nccl = comm->local[k].nccl;
    s->by_rank[x.rank] = &x;
    hipError_t e = hipSetDevice(x.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&x.compute, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&x.comm, hipStreamNonBlocking);
    for (hipEvent_t* ev : {&x.ev_ready, &x.ev_gather, &x.ev_read, &x.ev_sent, &x.ev_aux})
      if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&x.t0);
    if (e == hipSuccess) e = hipEventCreate(&x.t1);
    auto dmalloc = [&](float4** p, size_t rows) {
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), rows * sizeof(float4));
      if (e == hipSuccess) e = hipMemset(*p, 0, rows * sizeof(float4));
    };
    dmalloc(&x.posm_all, all);
    dmalloc(&x.vel, S);
    dmalloc(&x.acc[0], S);
    dmalloc(&x.acc[1], S);
    dmalloc(&x.mine, S);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&x.esum), 2 * (size_t)s->W * sizeof(double));
    x.plan = &s->plan.rank[(size_t)x.rank];
    x.send.assign(x.plan->tasks.size(), nullptr);
    x.recv.assign(x.plan->incoming.size(), nullptr);
    for (size_t t = 0; t < x.send.size(); t++) dmalloc(&x.send[t], x.plan->tasks[t].j1 - x.plan->tasks[t].j0);
    for (size_t b = 0; b < x.recv.size(); b++) dmalloc(&x.recv[b], x.plan->incoming[b].j1 - x.plan->incoming[b].j0);
    const InRanges ranges = in_ranges(*x.plan);
    x.in.n = ranges.n;
    for (int b = 0; b < ranges.n; b++) {
      x.in.buf[b] = x.recv[(size_t)b];
      x.in.j0[b] = ranges.j0[b];
      x.in.j1[b] = ranges.j1[b];
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(NBH_FAIL(e == hipErrorOutOfMemory ? NBODY_HIP_ERR_RESOURCE : NBODY_HIP_ERR_DEVICE,
                           "sharded Direct system, rank %d on device %d: %s", x.rank, x.device, hipGetErrorString(e)));
    }
    if (int rc = nbody_hip_ctx_create(&x.ctx, x.device, x.compute)) return fail(rc);
  }
  *out = s;
  return NBODY_HIP_OK;
}

// every local rank: upload its range of the whole-system host arrays
extern "C" int nbody_hip_sharded_direct_set_state(nbody_hip_sharded_direct* s, const float* x, const float* y,
                                                  const float* z, const float* mass, const float* vx,
                                                  const float* vy, const float* vz) {
  NBH_DIRECT_ENTER(s);
  if (!x || !y || !z || !mass) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null argument");
  if ((vx || vy || vz) && !(vx && vy && vz)) return NBH_FAIL(NBODY_HIP_ERR_STATE, "velocity arrays: all three or none");
  const size_t S = s->S;
  std::vector<float4> p(S), v(S);
  for (auto& sh : s->sh) {
    const ShardBounds b = shard_bounds(s->n, s->W, sh.rank);
    for (size_t i = 0; i < S; i++) {
      const size_t g = b.lo + i;
      const bool real = g < b.hi;
      p[i] = real ? make_float4(x[g], y[g], z[g], mass[g]) : make_float4(0.f, 0.f, 0.f, 0.f);  // padding: zero mass
      v[i] = real && vx ? make_float4(vx[g], vy[g], vz[g], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    NBH_HIP(hipSetDevice(sh.device));
    NBH_HIP(hipStreamSynchronize(sh.compute));
    NBH_HIP(hipStreamSynchronize(sh.comm));
    NBH_HIP(hipMemcpy(s->own(sh), p.data(), S * sizeof(float4), hipMemcpyHostToDevice));
    NBH_HIP(hipMemcpy(sh.vel, v.data(), S * sizeof(float4), hipMemcpyHostToDevice));
    NBH_HIP(hipMemset(sh.acc[0], 0, S * sizeof(float4)));
    NBH_HIP(hipMemset(sh.acc[1], 0, S * sizeof(float4)));
  }
  s->cur = 0;
  s->have_state = true;
  return NBODY_HIP_OK;
}

// ---- the transport ----------------------------------------------------------------------------------------------------
namespace {

using Sys = nbody_hip_sharded_direct;
nbody_float4* f4(float4* p) { return reinterpret_cast<nbody_float4*>(p); }

// a per-rank array of S rows, and the [W S] array of a rank that the gather fills
using RowsOf = float4* (*)(Sys*, Shard&);
float4* own_rows(Sys* s, Shard& x) { return s->own(x); }
float4* posm_all(Sys*, Shard& x) { return x.posm_all; }
float4* vel_rows(Sys*, Shard& x) { return x.vel; }
float4* acc_rows(Sys* s, Shard& x) { return x.acc[s->cur]; }
float4* stage_all(Sys*, Shard& x) { return x.stage; }
enum class Into { kEveryRank, kFirstRank };

// The transport, chosen ONCE per call: what this file needs from it.  Every peer, count and slot of the reaction exchange
// comes from the plan (shard_plan.h).
struct Link {
  Sys* s;
  explicit Link(Sys* sys) : s(sys) {}
  virtual ~Link() = default;
  // S rows of every rank -> rank r's rows of the [W S] array, on the comm streams.  What only the peer copies need: `guard`,
  // an event of the RECEIVING rank that its array may be overwritten after (nullptr: none), and whether every local rank
  // wants the array or only the first (RCCL fills every rank's).  Rows that already lie in place are not copied.
  virtual int all_gather(RowsOf src, RowsOf dst, hipEvent_t Shard::*guard, Into into) = 0;
  virtual int move_reactions() = 0;           // every task's send block -> its slot on the receiving rank, on the comm streams
  virtual int await_gather(Shard& x) = 0;     // x.compute waits for what all_gather brings (ev_gather on the comm streams)
  virtual int await_reactions(Shard& x) = 0;  // x.compute waits for what move_reactions brings (ev_sent on the comm streams)
};

// RCCL.  Peers match sends and receives in order: every rank issues its sends, in task order, before its receives, in
// incoming order (shard_plan_check: between two ranks that is at most one message each way).
struct RcclLink final : Link {
  Rccl* api;
  RcclLink(Sys* sys, Rccl* a) : Link(sys), api(a) {}
  template <class T>
  int all_gather_of(T* (*src)(Sys*, Shard&), T* (*dst)(Sys*, Shard&), size_t count, ncclDataType_t type) {
    NBH_NCCL_GROUP_START(api, s->sh.size());
    for (auto& x : s->sh) {
      NBH_HIP(hipSetDevice(x.device));
      NBH_NCCL(api, api->AllGather(src(s, x), dst(s, x), count, type, x.nccl, x.comm));
    }
    NBH_NCCL_GROUP_END(api, s->sh.size());
    return NBODY_HIP_OK;
  }
  int all_gather(RowsOf src, RowsOf dst, hipEvent_t Shard::*, Into) override {
    return all_gather_of<float4>(src, dst, s->S * 4, ncclFloat);
  }
  int move_reactions() override {
    NBH_NCCL(api, api->GroupStart());
    for (auto& x : s->sh) {
      NBH_HIP(hipSetDevice(x.device));
      for (size_t k = 0; k < x.send.size(); k++) {
        const ShardTask& t = x.plan->tasks[k];
        NBH_NCCL(api, api->Send(x.send[k], (t.j1 - t.j0) * 4, ncclFloat, t.shard, x.nccl, x.comm));
      }
      for (size_t k = 0; k < x.recv.size(); k++) {
        const ShardIncoming& in = x.plan->incoming[k];
        NBH_NCCL(api, api->Recv(x.recv[k], (in.j1 - in.j0) * 4, ncclFloat, in.from, x.nccl, x.comm));
      }
    }
    NBH_NCCL(api, api->GroupEnd());
    return NBODY_HIP_OK;
  }
  int await_gather(Shard& x) override {
    NBH_HIP(hipStreamWaitEvent(x.compute, x.ev_gather, 0));
    return NBODY_HIP_OK;
  }
  int await_reactions(Shard& x) override {
    NBH_HIP(hipStreamWaitEvent(x.compute, x.ev_sent, 0));
    return NBODY_HIP_OK;
  }
};

// One process driving all devices: the sender copies into the receiver's array on its own comm stream.
struct PeerLink final : Link {
  using Link::Link;
  int all_gather(RowsOf src, RowsOf dst, hipEvent_t Shard::*guard, Into into) override {
    const size_t S = s->S;
    for (auto& x : s->sh) {
      NBH_HIP(hipSetDevice(x.device));
      for (auto& p : s->sh) {
        float4* to = dst(s, p) + (size_t)x.rank * S;
        if (to == src(s, x) || (into == Into::kFirstRank && &p != &s->sh[0])) continue;
        if (guard) NBH_HIP(hipStreamWaitEvent(x.comm, p.*guard, 0));
        NBH_HIP(hipMemcpyAsync(to, src(s, x), S * sizeof(float4), hipMemcpyDeviceToDevice, x.comm));
      }
    }
    return NBODY_HIP_OK;
  }
  int move_reactions() override {
    for (auto& x : s->sh) {
      NBH_HIP(hipSetDevice(x.device));
      for (size_t k = 0; k < x.send.size(); k++) {
        const ShardTask& t = x.plan->tasks[k];
        NBH_HIP(hipMemcpyAsync(s->by_rank[t.shard]->recv[(size_t)t.slot], x.send[k], (t.j1 - t.j0) * sizeof(float4),
                               hipMemcpyDeviceToDevice, x.comm));
      }
    }
    return NBODY_HIP_OK;
  }
  int await_gather(Shard& x) override {
    for (auto& p : s->sh)
      if (&p != &x) NBH_HIP(hipStreamWaitEvent(x.compute, p.ev_gather, 0));
    return NBODY_HIP_OK;
  }
  int await_reactions(Shard& x) override {
    for (const ShardIncoming& b : x.plan->incoming) NBH_HIP(hipStreamWaitEvent(x.compute, s->by_rank[b.from]->ev_sent, 0));
    return NBODY_HIP_OK;
  }
};

// `body(link)` with the link of the call: RCCL when `rccl`, peer copies otherwise
template <class F>
int with_link(Sys* s, bool rccl, F body) {
  if (!rccl) {
    PeerLink link(s);
    return body(link);
  }
  Rccl* api = rccl_load();
  if (!api) return NBH_FAIL((nbody_hip_status)NBODY_HIP_ERR_COMM, "librccl.so.1 is not loaded");
  RcclLink link(s, api);
  return body(link);
}

int record_on_comm(Sys* s, hipEvent_t Shard::*ev) {
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipEventRecord(x.*ev, x.comm));
  }
  return NBODY_HIP_OK;
}

// the lazily allocated [W S] array of the read-backs
int stage_reserve(Sys* s, Shard& x) {
  if (x.stage) return NBODY_HIP_OK;
  NBH_HIP(hipStreamSynchronize(x.compute));
  NBH_HIP(hipMalloc(reinterpret_cast<void**>(&x.stage), s->S * (size_t)s->W * sizeof(float4)));
  return NBODY_HIP_OK;
}

// ---- one exchange + force evaluation, stage by stage ---------------------------------------------------------------
// -- 1: every rank's drifted rows -> every rank's posm_all, on the comm streams
int stage_gather(Sys* s, Link& link) {
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipEventRecord(x.ev_ready, x.compute));
    NBH_HIP(hipStreamWaitEvent(x.comm, x.ev_ready, 0));
  }
  // (peer copies: p's kernels of the last phase still read p.posm_all until p.ev_read)
  if (int rc = link.all_gather(own_rows, posm_all, &Shard::ev_read, Into::kEveryRank)) return rc;
  return record_on_comm(s, &Shard::ev_gather);
}

// -- 2: own x own -> mine (overlaps the gather)
int stage_own(Sys* s) {
  for (auto& x : s->sh)
    if (int rc = nbody_hip_direct_forces_packed(x.ctx, f4(s->own(x)), s->S, f4(s->own(x)), s->S, f4(x.mine), s->G, s->eps2, 0)) return rc;
  return NBODY_HIP_OK;
}

// -- 3: the compute streams wait for the gathered bodies
int stage_await_gather(Sys* s, Link& link) {
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    if (int rc = link.await_gather(x)) return rc;
  }
  return NBODY_HIP_OK;
}

// -- 4: the other shards, added to mine.  Pair mode: every task's two-set kernel, reactions -> the task's send block;
// otherwise the one-sided kernel against the shards left and right of the own range (tiny softening)
int stage_cross(Sys* s) {
  const size_t S = s->S, all = S * (size_t)s->W;
  for (auto& x : s->sh) {
    if (s->pair_mode) {
      for (size_t k = 0; k < x.send.size(); k++) {
        const ShardTask& t = x.plan->tasks[k];
        if (int rc = nbody_hip_direct_forces_pair_packed(x.ctx, f4(s->own(x) + t.i0), t.i1 - t.i0,
                                                         f4(x.posm_all + (size_t)t.shard * S + t.j0), t.j1 - t.j0,
                                                         f4(x.mine + t.i0), 1, f4(x.send[k]), 0, s->G, s->eps2))
          return rc;
      }
    } else if (s->W > 1) {
      const size_t r = (size_t)x.rank;
      if (r > 0)
        if (int rc = nbody_hip_direct_forces_packed(x.ctx, f4(s->own(x)), S, f4(x.posm_all), r * S, f4(x.mine), s->G, s->eps2, 1))
          return rc;
      if (r + 1 < (size_t)s->W)
        if (int rc = nbody_hip_direct_forces_packed(x.ctx, f4(s->own(x)), S, f4(x.posm_all + (r + 1) * S), all - (r + 1) * S,
                                                    f4(x.mine), s->G, s->eps2, 1))
          return rc;
    }
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipEventRecord(x.ev_read, x.compute));
  }
  return NBODY_HIP_OK;
}

// -- 5: pair mode: the reaction blocks -> their slots on the ranks they act on, on the comm streams
int stage_reactions(Sys* s, Link& link) {
  if (!s->pair_mode) return NBODY_HIP_OK;
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipStreamWaitEvent(x.comm, x.ev_read, 0));
  }
  if (int rc = link.move_reactions()) return rc;
  return record_on_comm(s, &Shard::ev_sent);
}

// -- 6: a_new = mine + the received blocks in ring-distance order.  kick: fused with v += (a_old + a_new) h, a_old =
// acc[cur], result -> acc[1 - cur]; otherwise result -> acc[out_slot]
int stage_finalize(Sys* s, Link& link, bool kick, float half_dt, int out_slot) {
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    if (s->pair_mode)
      if (int rc = link.await_reactions(x)) return rc;
    float4* a_new = kick ? x.acc[1 - s->cur] : x.acc[out_slot];
    hipLaunchKernelGGL(shard_finalize_kernel, dim3((unsigned)((s->S + kBlock - 1) / kBlock)), dim3(kBlock), 0, x.compute, x.mine,
                       x.in, (int)s->S, a_new, x.vel, x.acc[s->cur], half_dt, kick ? 1 : 0);
    NBH_LAUNCH_CHECK();
  }
  return NBODY_HIP_OK;
}

// gathered: posm_all already holds every shard on every rank (compute_forces)
int force_phase(Sys* s, Link& link, bool gathered, bool kick, float half_dt, int out_slot) {
  if (!gathered)
    if (int rc = stage_gather(s, link)) return rc;
  if (int rc = stage_own(s)) return rc;
  if (!gathered)
    if (int rc = stage_await_gather(s, link)) return rc;
  if (int rc = stage_cross(s)) return rc;
  if (int rc = stage_reactions(s, link)) return rc;
  return stage_finalize(s, link, kick, half_dt, out_slot);
}

bool by_rccl(const Sys* s) { return s->comm->transport == NBODY_HIP_TRANSPORT_RCCL; }

}  // namespace

extern "C" int nbody_hip_sharded_direct_forces(nbody_hip_sharded_direct* s) {
  NBH_DIRECT_ENTER_WITH_STATE(s, "no body state (call nbody_hip_sharded_direct_set_state first)");
  return with_link(s, by_rccl(s), [&](Link& link) { return force_phase(s, link, false, false, 0.f, s->cur); });
}

static int one_step(Sys* s, Link& link, float dt) {
  for (auto& x : s->sh)
    if (int rc = nbody_hip_drift_packed(x.ctx, f4(s->own(x)), f4(x.vel), f4(x.acc[s->cur]), s->S, dt)) return rc;
  if (int rc = force_phase(s, link, false, true, 0.5f * dt, 0)) return rc;
  s->cur = 1 - s->cur;  // a_old <- a by buffer swap
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_sharded_direct_step(nbody_hip_sharded_direct* s, float dt, int steps) {
  NBH_DIRECT_ENTER_WITH_STATE(s, "no body state (call nbody_hip_sharded_direct_set_state first)");
  if (!(dt > 0.0f) || !(dt <= 1.0f)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Time step must be in range (0, 1]");
  return with_link(s, by_rccl(s), [&](Link& link) {
    for (int k = 0; k < steps; k++)
      if (int rc = one_step(s, link, dt)) return rc;
    return (int)NBODY_HIP_OK;
  });
}

extern "C" int nbody_hip_sharded_direct_synchronize(nbody_hip_sharded_direct* s) {
  NBH_DIRECT_ENTER(s);
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipStreamSynchronize(x.comm));
    NBH_HIP(hipStreamSynchronize(x.compute));
  }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_sharded_direct_time_steps(nbody_hip_sharded_direct* s, float dt, int warmup, int steps,
                                                   float* ms_per_step) {
  nbh::DeviceGuard dev_guard;  // the caller's current device is restored on return
  if (!s || !ms_per_step) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null argument");
  if (steps <= 0 || warmup < 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "bad timing arguments");
  if (int rc = nbody_hip_sharded_direct_step(s, dt, warmup)) return rc;
  if (int rc = nbody_hip_sharded_direct_synchronize(s)) return rc;
  Shard& x = s->sh[0];
  NBH_HIP(hipSetDevice(x.device));
  NBH_HIP(hipEventRecord(x.t0, x.compute));
  if (int rc = nbody_hip_sharded_direct_step(s, dt, steps)) return rc;
  NBH_HIP(hipSetDevice(x.device));
  NBH_HIP(hipEventRecord(x.t1, x.compute));
  if (int rc = nbody_hip_sharded_direct_synchronize(s)) return rc;
  float ms = 0.f;
  NBH_HIP(hipEventElapsedTime(&ms, x.t0, x.t1));
  *ms_per_step = ms / (float)steps;
  return NBODY_HIP_OK;
}

// all-gather of a per-shard [S] float4 array into `stage` [W S] on every local rank (blocking)
static int gather_rows(Sys* s, Link& link, RowsOf src) {
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    if (int rc = stage_reserve(s, x)) return rc;
    NBH_HIP(hipStreamSynchronize(x.compute));
    NBH_HIP(hipStreamSynchronize(x.comm));
  }
  if (int rc = link.all_gather(src, stage_all, nullptr, Into::kEveryRank)) return rc;
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipStreamSynchronize(x.comm));
  }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_sharded_direct_get_state(nbody_hip_sharded_direct* s, float* x, float* y, float* z, float* vx,
                                                  float* vy, float* vz, float* ax, float* ay, float* az, int gather) {
  NBH_DIRECT_ENTER_WITH_STATE(s, "no body state");
  if (int rc = nbody_hip_sharded_direct_synchronize(s)) return rc;
  const size_t S = s->S, n = s->n;
  const bool whole = gather != 0 && !s->comm->all_local();
  std::vector<float4> h(whole ? S * (size_t)s->W : S);
  auto scatter = [&](float* a, float* b, float* c, size_t lo, size_t count, const float4* src) {
    for (size_t i = 0; i < count; i++) {
      if (a) a[lo + i] = src[i].x;
      if (b) b[lo + i] = src[i].y;
      if (c) c[lo + i] = src[i].z;
    }
  };
  if (whole) {
    // positions: posm_all of any local rank holds every shard as of the last exchange (= the current positions);
    // velocities and accelerations are all-gathered
    Shard& r0 = s->sh[0];
    NBH_HIP(hipSetDevice(r0.device));
    if (x || y || z) {
      NBH_HIP(hipMemcpy(h.data(), r0.posm_all, h.size() * sizeof(float4), hipMemcpyDeviceToHost));
      scatter(x, y, z, 0, n, h.data());
    }
    for (int which = 0; which < 2; which++) {
      float *a = which ? ax : vx, *b = which ? ay : vy, *c = which ? az : vz;
      if (!a && !b && !c) continue;
      if (int rc = with_link(s, by_rccl(s), [&](Link& link) { return gather_rows(s, link, which ? acc_rows : vel_rows); })) return rc;
      NBH_HIP(hipSetDevice(r0.device));
      NBH_HIP(hipMemcpy(h.data(), r0.stage, h.size() * sizeof(float4), hipMemcpyDeviceToHost));
      scatter(a, b, c, 0, n, h.data());
    }
    return NBODY_HIP_OK;
  }
  for (auto& sh : s->sh) {
    const ShardBounds own = shard_bounds(n, s->W, sh.rank);
    const size_t lo = own.lo, hi = own.hi;
    NBH_HIP(hipSetDevice(sh.device));
    if (x || y || z) {
      NBH_HIP(hipMemcpy(h.data(), s->own(sh), S * sizeof(float4), hipMemcpyDeviceToHost));
      scatter(x, y, z, lo, hi - lo, h.data());
    }
    if (vx || vy || vz) {
      NBH_HIP(hipMemcpy(h.data(), sh.vel, S * sizeof(float4), hipMemcpyDeviceToHost));
      scatter(vx, vy, vz, lo, hi - lo, h.data());
    }
    if (ax || ay || az) {
      NBH_HIP(hipMemcpy(h.data(), sh.acc[s->cur], S * sizeof(float4), hipMemcpyDeviceToHost));
      scatter(ax, ay, az, lo, hi - lo, h.data());
    }
  }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_sharded_direct_energies(nbody_hip_sharded_direct* s, double* kinetic, double* potential) {
  NBH_DIRECT_ENTER_WITH_STATE(s, "no body state");
  if (int rc = nbody_hip_sharded_direct_synchronize(s)) return rc;
  const size_t S = s->S, all = S * (size_t)s->W;
  const int W = s->W;
  std::vector<double> e(2 * (size_t)W, 0.0);
  // posm_all holds every shard as of the last exchange (nothing moves bodies after the drift of a step)
  for (auto& x : s->sh) {
    double out[2];
    if (int rc = nbody_hip_energies_packed(x.ctx, f4(s->own(x)), f4(x.vel), S, (long long)((size_t)x.rank * S), f4(x.posm_all), all,
                                           s->G, s->eps, out))
      return rc;
    e[2 * (size_t)x.rank] = out[0];
    e[2 * (size_t)x.rank + 1] = out[1];
  }
  if (!s->comm->all_local()) {  // one process per GPU (RCCL): all-gather the 2 doubles of every rank, then sum in rank order
    Rccl* api = rccl_load();
    if (!api) return NBH_FAIL((nbody_hip_status)NBODY_HIP_ERR_COMM, "librccl.so.1 is not loaded");
    for (auto& x : s->sh) {
      NBH_HIP(hipSetDevice(x.device));
      NBH_HIP(hipMemcpyAsync(x.esum + 2 * (size_t)x.rank, &e[2 * (size_t)x.rank], 2 * sizeof(double), hipMemcpyHostToDevice, x.comm));
    }
    if (int rc = RcclLink(s, api).all_gather_of<double>([](Sys*, Shard& x) { return x.esum + 2 * (size_t)x.rank; },
                                                        [](Sys*, Shard& x) { return x.esum; }, 2, ncclDouble))
      return rc;
    Shard& r0 = s->sh[0];
    NBH_HIP(hipSetDevice(r0.device));
    NBH_HIP(hipStreamSynchronize(r0.comm));
    NBH_HIP(hipMemcpy(e.data(), r0.esum, e.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (auto& x : s->sh) {
      NBH_HIP(hipSetDevice(x.device));
      NBH_HIP(hipStreamSynchronize(x.comm));
    }
  }
  double ke = 0.0, pe = 0.0;
  for (int r = 0; r < W; r++) {
    ke += e[2 * (size_t)r];
    pe += e[2 * (size_t)r + 1];
  }
  if (kinetic) *kinetic = ke;
  if (potential) *potential = pe;
  return NBODY_HIP_OK;
}

// the plugin form: the whole system in d (SoA, on the first local rank's device) -> d->acc_*
extern "C" int nbody_hip_sharded_direct_compute_forces(nbody_hip_sharded_direct* s, nbody_particle_data* d) {
  NBH_DIRECT_ENTER(s);
  if (!d) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null particle data");
  if (d->count != s->n) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle count %zu does not match the system's %zu", d->count, s->n);
  if (!d->pos_x || !d->pos_y || !d->pos_z || !d->mass || !d->acc_x || !d->acc_y || !d->acc_z)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null arrays");
  const size_t n = s->n;
  Shard& r0 = s->sh[0];
  NBH_HIP(hipSetDevice(r0.device));
  // order against the caller's work on the null stream of that device (the reference's threading model:
  // everything on the null stream, force_calculator.hpp:8-19)
  NBH_HIP(hipEventRecord(r0.ev_aux, nullptr));
  NBH_HIP(hipStreamWaitEvent(r0.compute, r0.ev_aux, 0));
  // the readers of the last phase on the other ranks must be done before their posm_all is overwritten
  for (auto& p : s->sh)
    if (&p != &r0) NBH_HIP(hipStreamWaitEvent(r0.compute, p.ev_read, 0));
  if (int rc = nbody_hip_pack_posm(r0.ctx, d->pos_x, d->pos_y, d->pos_z, d->mass, n, f4(r0.posm_all)))
    return rc;
  NBH_HIP(hipEventRecord(r0.ev_ready, r0.compute));
  for (auto& p : s->sh) {
    if (&p == &r0) continue;
    NBH_HIP(hipMemcpyAsync(p.posm_all, r0.posm_all, n * sizeof(float4), hipMemcpyDeviceToDevice, r0.compute));
  }
  NBH_HIP(hipEventRecord(r0.ev_gather, r0.compute));
  for (auto& p : s->sh) {
    if (&p == &r0) continue;
    NBH_HIP(hipSetDevice(p.device));
    NBH_HIP(hipStreamWaitEvent(p.compute, r0.ev_gather, 0));
  }
  s->have_state = true;  // (positions only: a resident step after this needs set_state for the velocities)
  if (int rc = with_link(s, by_rccl(s), [&](Link& link) { return force_phase(s, link, true, false, 0.f, s->cur); })) return rc;
  // accelerations of every shard -> stage of the first local rank -> d->acc_*
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    if (int rc = stage_reserve(s, x)) return rc;
    NBH_HIP(hipEventRecord(x.ev_ready, x.compute));
    NBH_HIP(hipStreamWaitEvent(x.comm, x.ev_ready, 0));
  }
  // (local ranks copy to the first one alone, whatever the transport; one process per GPU has only RCCL)
  if (int rc = with_link(s, !s->comm->all_local(), [&](Link& link) { return link.all_gather(acc_rows, stage_all, nullptr, Into::kFirstRank); }))
    return rc;
  for (auto& x : s->sh) {
    NBH_HIP(hipSetDevice(x.device));
    NBH_HIP(hipEventRecord(x.ev_sent, x.comm));
    NBH_HIP(hipSetDevice(r0.device));
    NBH_HIP(hipStreamWaitEvent(r0.compute, x.ev_sent, 0));
  }
  if (int rc = nbody_hip_unpack3(r0.ctx, f4(r0.stage), n, d->acc_x, d->acc_y, d->acc_z)) return rc;
  NBH_HIP(hipEventRecord(r0.ev_aux, r0.compute));
  NBH_HIP(hipStreamWaitEvent(nullptr, r0.ev_aux, 0));
  return NBODY_HIP_OK;
}
