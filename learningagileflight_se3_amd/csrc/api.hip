// api.hip — extern "C" boundary of liblafse3.so (declared in include/lafse3.h).
//
// Host side only: argument checking, workspace management, kernel launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "lafse3.h"

namespace lafse3 {
struct KernelArgs;
}

// kernels (#included so the whole library is one translation unit)
#include "ipm_kernel.hip"   // wave-per-instance solver (the only variant; params.variant must be WAVE)
#include "moving.hip"       // traversal-time fixed point of the moving-gate loop

namespace {

thread_local std::string g_err;

int fail(int code, const char *what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    else
        snprintf(buf, sizeof(buf), "%s", what);
    g_err = buf;
    return code;
}

// Makes `dev` the calling thread's current HIP device for a scope and puts the caller's device (torch's) back on
// every return path.  `err` is the result of the switch; an entry point whose switch failed returns LAFSE3_EDEVICE.
struct DeviceGuard {
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        if (prev_ == dev) prev_ = -1;   // already there: nothing to switch, nothing to put back
        else err = hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev_ >= 0) (void)hipSetDevice(prev_); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;

private:
    int prev_ = -1;
};

// Grow-only device array, freed with its owner.  Growing is hipFree then hipMalloc, and stays so: the blocking
// hipFree synchronises the device, which is what makes growing safe while an earlier launch on another stream still
// uses the old array (a stream-ordered free or allocation would not wait for it).  Contents are not kept.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    hipError_t ensure(int64_t n)
    {
        if (n <= cap_) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p_, (size_t)n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    T *data() const { return p_; }
    int64_t capacity() const { return cap_; }

private:
    T *p_ = nullptr;
    int64_t cap_ = 0;   // elements
};

}  // namespace

struct lafse3_ctx {
    int device = 0;
    lafse3_params prm{};
    DevBuf<double> ws, rws;              // solver and restoration-phase workspace (WS_SIZE / RWS_SIZE per slot)
    DevBuf<double> tmp;                  // rewards9 scratch for sol_gradient, control trajectory of get_input
    DevBuf<double> tmp32;                // fp64 staging of the fp32 twin (lafse3_ocp_solve_f32)
    DevBuf<unsigned long long> counters;   // [0..2] iteration / sweep / trial totals, [3] work-queue head,
                                           // [4] device error word (ipm_kernel.hip ERR_*: kept until
                                           // lafse3_check_device reports it), [5..6] restoration counts;
                                           // words N_COUNTERS.. are trajectory scoring's (lafse3_reward)
    int64_t slots = 0;                         // resident solver waves: CUs x 4 SIMDs x waves per SIMD
    DevBuf<unsigned> sched;                    // sol_gradient probe queue (ipm_kernel.hip sched_next)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    double *trace = nullptr;   // debug trace target (device), see lafse3_debug_trace
    int trace_iters = 0;
    double *dump = nullptr;
    int dump_it = -1, dump_refine = 0;
    lafse3::RestoDumpArgs rdump = {nullptr, -1, -1, 0};
    unsigned long long *ptime = nullptr;
    int32_t *iters_rec = nullptr;        // lafse3_record_iters target (device)
    int64_t iters_cap = 0;               // its capacity in entries
    int64_t drop_push = -1;              // debug: lafse3_debug_drop_push
    // private stream of the context: the counters of the last solver launch are read (and its error word cleared)
    // here after ev1 has completed, never on the caller's launch stream, which the caller may have destroyed since
    hipStream_t aux = nullptr;

    ~lafse3_ctx()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (aux) (void)hipStreamDestroy(aux);
    }
};

using lafse3::N_COUNTERS;
static_assert(N_COUNTERS > lafse3::CNT_ERR && N_COUNTERS > lafse3::CNT_RESTO + 1,
              "N_COUNTERS must cover the error word and both restoration counts");
static size_t ws_doubles(int64_t n) { return (size_t)n * (size_t)lafse3::WS_SIZE; }

// The flat one-dimensional helper launches: one thread per element of n, 256 per block.
template <typename K, typename... Args>
static int launch_flat(K kernel, int64_t n, hipStream_t st, const char *what, Args... args)
{
    const int tpb = 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + tpb - 1) / tpb)), dim3(tpb), 0, st, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LAFSE3_OK : fail(LAFSE3_EDEVICE, what, e);
}

// Opening of the solver and scoring entry points: the context and batch, the pointers a non-empty batch needs, and
// the one-launch limit on B x per NLP instances (the kernels index instances with 32 bits).
static int check_call(const lafse3_ctx *c, int64_t B, std::initializer_list<const void *> required, int per = 1)
{
    if (!c || B < 0) return fail(LAFSE3_EINVAL, "bad ctx / batch");
    for (const void *p : required)
        if (B > 0 && !p) return fail(LAFSE3_EINVAL, "null argument");
    if (B > 0x7fffffffLL / per) return fail(LAFSE3_EINVAL, "batch too large for one launch");
    return LAFSE3_OK;
}

// The reward's goal path term reads rows N-4..N-1 of the N+1 trajectory rows with numpy's wrap of negative rows
// (quad_policy.py:88-89; ipm_kernel.hip reward_fused).  At horizon 1 the reference indexes row -3 of two rows and
// raises: the entry points that score a reward refuse that horizon before any allocation or launch.
static int check_reward_horizon(const lafse3_ctx *c, const char *entry)
{
    if (c->prm.horizon >= 2) return LAFSE3_OK;
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: the reward is undefined at horizon %d: its goal path term reads row N-4 of the N+1 "
             "trajectory rows, which the reference cannot index below horizon 2", entry, (int)c->prm.horizon);
    return fail(LAFSE3_EINVAL, buf);
}

extern "C" {

int lafse3_default_params(lafse3_params *p)
{
    if (!p) return fail(LAFSE3_EINVAL, "null params");
    std::memset(p, 0, sizeof(*p));
    p->mass = 0.5; p->Jx = 0.0023; p->Jy = 0.0023; p->Jz = 0.004;          // quad_policy.py:37
    p->arm_l = 0.35; p->c_tau = 0.0245; p->grav = 9.78; p->dt = 0.1;        // quad_model.py:37, quad_policy.py:43
    p->wrt = 5; p->wqt = 80; p->wthrust = 0.1; p->wrf = 5; p->wvf = 5; p->wqf = 0; p->wwf = 3;  // quad_policy.py:38
    p->tra_w_peak = 60; p->tra_w_decay = 10; p->du_weight = 1;             // quad_OC.py:145,150
    p->u_lb = 0; p->u_ub = 2 * 1.22;                                        // quad_policy.py:48-51
    p->w_lb = -3.141592653589793 / 2; p->w_ub = 3.141592653589793 / 2;      // quad_policy.py:47,50
    p->wing_len = 1.5; p->d_min = 0.2;                                      // quad_policy.py:19, solid_geometry.py:115
    p->horizon = 50;                                                        // quad_policy.py:17
    p->max_iter = 3000; p->tol = 1e-8; p->acceptable_tol = 1e-6; p->acceptable_iter = 15;  // IPOPT defaults
    p->mu_init = 0.1; p->bound_relax = 1e-8; p->lsq_mult_init = 1;
    p->variant = LAFSE3_VARIANT_WAVE;
    p->max_soc = 4;
    p->costate_option = 0;
    p->grad_mode = 0;
    p->restoration = 1;
    p->watchdog = 10;
    return LAFSE3_OK;
}

int64_t lafse3_workspace_bytes_per_instance(void)
{
    return (int64_t)((ws_doubles(1) + (size_t)lafse3::RWS_SIZE) * sizeof(double));
}

int lafse3_stream_create(int device, void **stream)
{
    if (!stream) return fail(LAFSE3_EINVAL, "null stream");
    *stream = nullptr;
    hipError_t e;
    if (device < 0 && (e = hipGetDevice(&device)) != hipSuccess) return fail(LAFSE3_EDEVICE, "hipGetDevice", e);
    DeviceGuard dev(device);
    int cus = 0;
    e = dev.err;
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess || cus <= 0) return fail(LAFSE3_EDEVICE, "CU count", e);
    // a CU-masked stream gets a hardware queue of its own (the runtime does not share masked queues); the mask
    // enables every CU, so the stream runs exactly as an ordinary one otherwise
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0xffffffffu);
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
    hipStream_t st = nullptr;
    e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipExtStreamCreateWithCUMask", e);
    *stream = (void *)st;
    return LAFSE3_OK;
}

int lafse3_stream_destroy(void *stream)
{
    if (!stream) return fail(LAFSE3_EINVAL, "null stream");
    const hipError_t e = hipStreamDestroy((hipStream_t)stream);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipStreamDestroy", e);
    return LAFSE3_OK;
}

int lafse3_create(lafse3_ctx **ctx, int device)
{
    if (!ctx) return fail(LAFSE3_EINVAL, "null ctx");
    hipError_t e;
    if (device < 0 && (e = hipGetDevice(&device)) != hipSuccess) return fail(LAFSE3_EDEVICE, "hipGetDevice", e);
    DeviceGuard dev(device);   // declared before c: a context abandoned below is destroyed on its own device
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    std::unique_ptr<lafse3_ctx> c(new lafse3_ctx());
    c->device = device;
    lafse3_default_params(&c->prm);
    e = c->counters.ensure(2 * N_COUNTERS);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMalloc counters", e);
    {
        // zeroed on a private stream and waited for there (a device-wide synchronize would also wait for other
        // contexts' solver launches in flight); complete before this call returns, so before any launch on it
        hipStream_t zs = nullptr;
        e = hipStreamCreateWithFlags(&zs, hipStreamNonBlocking);
        if (e == hipSuccess)
            e = hipMemsetAsync(c->counters.data(), 0, 2 * N_COUNTERS * sizeof(unsigned long long), zs);
        if (e == hipSuccess) e = hipStreamSynchronize(zs);
        if (zs) (void)hipStreamDestroy(zs);
    }
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemset counters", e);
    int cus = 0;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    if (e != hipSuccess || cus <= 0) return fail(LAFSE3_EDEVICE, "hipDeviceGetAttribute(CU count)", e);
    c->slots = (int64_t)cus * 4;   // one wave per SIMD (ipm_kernel __launch_bounds__(64, 1))
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking)) != hipSuccess)
        return fail(LAFSE3_EDEVICE, "hipEventCreate / hipStreamCreate", e);
    *ctx = c.release();
    return LAFSE3_OK;
}

int lafse3_destroy(lafse3_ctx *c)
{
    if (!c) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    delete c;
    return LAFSE3_OK;
}

static int check_params(const lafse3_params *p)
{
    if (p->horizon < 1 || p->horizon > LAFSE3_MAX_N) return fail(LAFSE3_EINVAL, "horizon must be in [1, 50]");
    if (!(p->u_ub > p->u_lb) || !(p->w_ub > p->w_lb)) return fail(LAFSE3_EINVAL, "empty bound box");
    if (p->variant != LAFSE3_VARIANT_WAVE)
        return fail(LAFSE3_EINVAL, "unknown kernel variant (the lane-per-instance variant was removed in 0.3)");
    if (!(p->dt > 0) || !(p->mass > 0) || !(p->Jx > 0) || !(p->Jy > 0) || !(p->Jz > 0))
        return fail(LAFSE3_EINVAL, "non-positive model constant");
    if (p->max_iter < 0 || !(p->tol > 0) || p->max_soc < 0) return fail(LAFSE3_EINVAL, "bad solver option");
    if (p->costate_option != 0 && p->costate_option != 1) return fail(LAFSE3_EINVAL, "costate_option must be 0 or 1");
    if (p->grad_mode != 0 && p->grad_mode != 1) return fail(LAFSE3_EINVAL, "grad_mode must be 0 (FD) or 1 (IFT)");
    if (p->restoration != 0 && p->restoration != 1) return fail(LAFSE3_EINVAL, "restoration must be 0 or 1");
    if (p->watchdog < 0) return fail(LAFSE3_EINVAL, "watchdog must be >= 0");
    return LAFSE3_OK;
}

int lafse3_set_params(lafse3_ctx *c, const lafse3_params *p)
{
    if (!c || !p) return fail(LAFSE3_EINVAL, "null argument");
    int rc = check_params(p);
    if (rc) return rc;
    c->prm = *p;
    return LAFSE3_OK;
}

int lafse3_get_params(const lafse3_ctx *c, lafse3_params *p)
{
    if (!c || !p) return fail(LAFSE3_EINVAL, "null argument");
    *p = c->prm;
    return LAFSE3_OK;
}

// probe queue of a sol_gradient launch of B samples: 2 NB + 1 counters + NB x B bucket slots
static int64_t sched_words(int64_t B) { return 2 * lafse3::SCHED_NB + 1 + lafse3::SCHED_NB * B; }

// workspace slots of n resident waves: ws and rws grow together, and a failed allocation leaves both empty
static int reserve_ws(lafse3_ctx *c, int64_t n)
{
    const char *what = "hipMalloc workspace";
    hipError_t e = c->ws.ensure((int64_t)ws_doubles(n));
    if (e == hipSuccess) {
        what = "hipMalloc restoration workspace";
        e = c->rws.ensure(n * lafse3::RWS_SIZE);
    }
    if (e == hipSuccess) return LAFSE3_OK;
    c->ws.release();
    c->rws.release();
    return fail(LAFSE3_EDEVICE, what, e);
}

int lafse3_reserve(lafse3_ctx *c, int64_t n)
{
    if (!c || n < 0) return fail(LAFSE3_EINVAL, "bad reserve");
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    if (n > 0) {   // the probe queue of a sol_gradient launch of up to n samples (n instances cover n / 9)
        const hipError_t e = c->sched.ensure(sched_words(n));
        if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMalloc probe queue", e);
    }
    return reserve_ws(c, n < c->slots ? n : c->slots);   // persistent solver: one workspace slot per resident wave
}

// rewards9 / status9 slots before a sol_gradient launch: NaN / ST_DEVICE_ERR, overwritten by every solve that
// runs, so a slot whose probe task was lost (ipm_kernel.hip sched_next) cannot pass for a result
__global__ void slots_init_kernel(double *R, int32_t *S, int64_t n)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= n) return;
    R[e] = __builtin_nan("");
    if (S) S[e] = lafse3::ST_DEVICE_ERR;
}

static int launch(lafse3_ctx *c, lafse3::KernelArgs &A, hipStream_t st, int64_t sched_samples = 0,
                  const lafse3::ExtArgs *ext = nullptr, const lafse3::WarmArgs *warm = nullptr)
{
    if (A.n_inst == 0) return LAFSE3_OK;
    // trajectory scoring (MODE_REWARD) counts nothing and has its own queue head: it leaves the last solver
    // launch's counters, error word, timing events and stream alone, and records no iteration counts
    const bool scoring = A.mode == lafse3::MODE_REWARD;
    if (!A.iters_out && c->iters_rec && !scoring) {
        // slots the kernel writes: b * 9 + j for sol_gradient (both gradient modes), the instance index otherwise
        const int64_t need = (A.mode == lafse3::MODE_GRAD) ? sched_samples * 9 : A.n_inst;
        if (need > c->iters_cap) {
            char buf[160];
            snprintf(buf, sizeof(buf), "lafse3_record_iters buffer holds %lld entries, this launch writes %lld",
                     (long long)c->iters_cap, (long long)need);
            return fail(LAFSE3_EINVAL, buf);
        }
        A.iters_out = c->iters_rec;
    }
    // persistent grid: one workgroup per SIMD slot (fewer when the batch is smaller), workspace per workgroup
    const int64_t grid = A.n_inst < c->slots ? A.n_inst : c->slots;
    const int rc = reserve_ws(c, grid);
    if (rc) return rc;
    A.persistent = 1;
    A.prm = c->prm;
    A.ws = c->ws.data();
    A.rws = c->rws.data();
    A.counters = c->counters.data() + (scoring ? N_COUNTERS : 0);
    A.trace = c->trace;
    A.trace_iters = c->trace_iters;
    A.ptime = c->ptime;
    A.dump = c->dump;
    A.dump_it = c->dump_it;
    A.dump_refine = c->dump_refine;
    A.drop_push = c->drop_push;
    // every word but the device error word, which stays set until lafse3_check_device has reported it
    hipError_t e = hipMemsetAsync(A.counters, 0, lafse3::CNT_ERR * sizeof(unsigned long long), st);
    if (e == hipSuccess)
        e = hipMemsetAsync(A.counters + lafse3::CNT_ERR + 1, 0,
                           (N_COUNTERS - lafse3::CNT_ERR - 1) * sizeof(unsigned long long), st);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemsetAsync", e);
    A.sched = nullptr;
    if (sched_samples > 0) {
        e = c->sched.ensure(sched_words(sched_samples));
        if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMalloc probe queue", e);
        e = hipMemsetAsync(c->sched.data(), 0, (size_t)sched_words(sched_samples) * sizeof(unsigned), st);
        if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemsetAsync probe queue", e);
        A.sched = c->sched.data();
    }
    if (scoring) {
        hipLaunchKernelGGL(lafse3::ipm_kernel, dim3((unsigned)grid), dim3(64), 0, st, A);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "scoring kernel launch", e);
        return LAFSE3_OK;
    }
    (void)hipEventRecord(c->ev0, st);
    // per-instance weights, the sensitivity pass and the optimum record are compiled into a kernel of their own
    // (ipm_kernel.hip ipm_kernel_ext), and so are the extra stores of a debug dump that carries the iterate
    // (ipm_kernel_dump: plain solves only); the warm start has ipm_kernel_ext's arguments and its own (ipm_kernel_warm)
    if (ext && warm)
        hipLaunchKernelGGL(lafse3::ipm_kernel_warm, dim3((unsigned)grid), dim3(64), 0, st, A, *ext, *warm);
    else if (ext) hipLaunchKernelGGL(lafse3::ipm_kernel_ext, dim3((unsigned)grid), dim3(64), 0, st, A, *ext);
    else if ((A.dump || c->rdump.buf) && A.mode == lafse3::MODE_SOLVE && !A.sched)
        hipLaunchKernelGGL(lafse3::ipm_kernel_dump, dim3((unsigned)grid), dim3(64), 0, st, A, c->rdump);
    else hipLaunchKernelGGL(lafse3::ipm_kernel, dim3((unsigned)grid), dim3(64), 0, st, A);
    e = hipGetLastError();
    (void)hipEventRecord(c->ev1, st);
    c->timed = true;
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "solver kernel launch", e);
    return LAFSE3_OK;
}

static lafse3::KernelArgs blank_args()
{
    lafse3::KernelArgs A;
    std::memset(&A, 0, sizeof(A));
    return A;
}

// lafse3_ocp_solve and, with ext, lafse3_ocp_sensitivity / _ex / _w / lafse3_ocp_solve_rec: the one place that fills the
// MODE_SOLVE arguments
static int solve(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                 const double *a_tra, const double *t, const double *u_last, double *x, double *u, double *lam,
                 double *cost, int32_t *status, int32_t *iters, void *stream, const lafse3::ExtArgs *ext,
                 const lafse3::WarmArgs *warm = nullptr)
{
    if (const int rc = check_call(c, B, {ini, goal, p_tra, a_tra, t})) return rc;
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    lafse3::KernelArgs A = blank_args();
    A.mode = lafse3::MODE_SOLVE;
    A.n_inst = B;
    A.ini = ini; A.goal = goal; A.ptra = p_tra; A.atra = a_tra; A.t = t; A.ulast = u_last;
    A.x_out = x; A.u_out = u; A.lam_out = lam; A.cost_out = cost; A.status_out = status; A.iters_out = iters;
    return launch(c, A, (hipStream_t)stream, 0, ext, warm);
}

int lafse3_ocp_solve(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                     const double *a_tra, const double *t, const double *u_last, double *x, double *u, double *lam,
                     double *cost, int32_t *status, int32_t *iters, void *stream)
{
    return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, nullptr);
}

int lafse3_ocp_sensitivity(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                           const double *a_tra, const double *t, const double *u_last, double *x, double *u,
                           double *lam, double *cost, int32_t *status, int32_t *iters, double *dx, double *du,
                           int32_t *sens_status, void *stream)
{
    lafse3::ExtArgs Z = {};
    Z.dx_out = dx; Z.du_out = du; Z.sens_out = sens_status; Z.groups = LAFSE3_SENS_THETA;
    // without dx and du the call is lafse3_ocp_solve
    return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream,
                 dx || du ? &Z : nullptr);
}

static_assert(LAFSE3_SENS_THETA == lafse3::SENS_G_THETA && LAFSE3_SENS_INI == lafse3::SENS_G_INI &&
              LAFSE3_SENS_GOAL == lafse3::SENS_G_GOAL, "sens.inc reads the header's group bits");

int lafse3_sens_columns(int32_t groups)
{
    if (groups & ~(LAFSE3_SENS_THETA | LAFSE3_SENS_INI | LAFSE3_SENS_GOAL))
        return fail(LAFSE3_EINVAL, "lafse3_sens_columns: bits outside LAFSE3_SENS_THETA | _INI | _GOAL");
    return lafse3::sens_columns(groups);
}

int lafse3_ocp_sensitivity_ex(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                              const double *a_tra, const double *t, const double *u_last, double *x, double *u,
                              double *lam, double *cost, int32_t *status, int32_t *iters, int32_t groups, double *dx,
                              double *du, double *gain, int32_t *sens_status, void *stream)
{
    if (!c) return fail(LAFSE3_EINVAL, "bad ctx / batch");
    // without dx, du and gain the call is lafse3_ocp_solve
    if (!dx && !du && !gain)
        return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, nullptr);
    if (groups == 0 || (groups & ~(LAFSE3_SENS_THETA | LAFSE3_SENS_INI | LAFSE3_SENS_GOAL)))
        return fail(LAFSE3_EINVAL, "lafse3_ocp_sensitivity_ex: groups must be a non-empty subset of "
                                   "LAFSE3_SENS_THETA | LAFSE3_SENS_INI | LAFSE3_SENS_GOAL");
    lafse3::ExtArgs Z = {};
    Z.dx_out = dx; Z.du_out = du; Z.gain_out = gain; Z.sens_out = sens_status; Z.groups = groups;
    return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, &Z);
}

static_assert(LAFSE3_SENS_WEIGHTS == lafse3::SENS_G_W && LAFSE3_NW == lafse3::NW,
              "sens.inc reads the header's weights group");
// the ten weights are contiguous doubles of lafse3_params in the column order (weight_columns.hpp)
static_assert(offsetof(lafse3_params, du_weight) - offsetof(lafse3_params, wrt) == (LAFSE3_NW - 1) * sizeof(double) &&
              offsetof(lafse3_params, tra_w_peak) - offsetof(lafse3_params, wrt) == lafse3::W_PEAK * sizeof(double),
              "lafse3_params: wrt .. du_weight are LAFSE3_NW contiguous doubles");

int lafse3_sens_columns_w(int32_t groups)
{
    if (groups & ~lafse3::SENS_W_ALL)
        return fail(LAFSE3_EINVAL, "lafse3_sens_columns_w: bits outside LAFSE3_SENS_THETA | _INI | _GOAL | _WEIGHTS");
    return lafse3::sens_columns(groups);
}

int lafse3_params_weights(const lafse3_params *p, double w[LAFSE3_NW])
{
    if (!p || !w) return fail(LAFSE3_EINVAL, "null argument");
    std::memcpy(w, &p->wrt, LAFSE3_NW * sizeof(double));
    return LAFSE3_OK;
}

int lafse3_ocp_sensitivity_w(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                             const double *a_tra, const double *t, const double *u_last, const double *weights,
                             double *x, double *u, double *lam, double *cost, int32_t *status, int32_t *iters,
                             int32_t groups, double *dx, double *du, double *gain, int32_t *sens_status, void *stream)
{
    if (!c) return fail(LAFSE3_EINVAL, "bad ctx / batch");
    const bool sens = dx || du || gain;
    // without dx, du, gain and weights the call is lafse3_ocp_solve
    if (!sens && !weights)
        return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, nullptr);
    if (sens && (groups == 0 || (groups & ~lafse3::SENS_W_ALL)))
        return fail(LAFSE3_EINVAL, "lafse3_ocp_sensitivity_w: groups must be a non-empty subset of "
                                   "LAFSE3_SENS_THETA | LAFSE3_SENS_INI | LAFSE3_SENS_GOAL | LAFSE3_SENS_WEIGHTS");
    lafse3::ExtArgs Z = {};
    Z.weights = weights;
    Z.dx_out = dx; Z.du_out = du; Z.gain_out = gain; Z.sens_out = sens_status;
    Z.groups = sens ? groups : 0;   // a plain solve with per-instance weights ignores groups
    return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, &Z);
}

int lafse3_rec_width(void) { return lafse3::REC_W; }

int lafse3_ocp_solve_rec(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                         const double *a_tra, const double *t, const double *u_last, const double *weights, double *x,
                         double *u, double *lam, double *cost, int32_t *status, int32_t *iters, double *rec,
                         void *stream)
{
    if (!c) return fail(LAFSE3_EINVAL, "bad ctx / batch");
    if (!rec) return fail(LAFSE3_EINVAL, "lafse3_ocp_solve_rec: rec is required");
    lafse3::ExtArgs Z = {};
    Z.weights = weights;
    Z.rec = rec;
    return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, &Z);
}

int lafse3_default_warm_opts(lafse3_warm_opts *o)
{
    if (!o) return fail(LAFSE3_EINVAL, "null warm opts");
    std::memset(o, 0, sizeof(*o));
    o->shift = 0;
    o->mu_init = 1e-3;
    o->bound_push = 1e-3; o->bound_frac = 1e-3; o->mult_bound_push = 1e-3;   // IPOPT warm_start_* defaults
    return LAFSE3_OK;
}

int lafse3_ocp_solve_warm(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                          const double *a_tra, const double *t, const double *u_last, const double *weights,
                          const double *rec_in, const lafse3_warm_opts *opts, double *x, double *u, double *lam,
                          double *cost, int32_t *status, int32_t *iters, int32_t *warm_status, double *rec_out,
                          void *stream)
{
    if (!c) return fail(LAFSE3_EINVAL, "bad ctx / batch");
    if (!rec_in) return fail(LAFSE3_EINVAL, "lafse3_ocp_solve_warm: rec_in is required");
    lafse3_warm_opts o;
    lafse3_default_warm_opts(&o);
    if (opts) o = *opts;
    if (o.shift < 0) return fail(LAFSE3_EINVAL, "lafse3_ocp_solve_warm: negative shift");
    if (!std::isfinite(o.mu_init) || !std::isfinite(o.bound_push) || !std::isfinite(o.bound_frac) ||
        !std::isfinite(o.mult_bound_push))
        return fail(LAFSE3_EINVAL, "lafse3_ocp_solve_warm: non-finite option");
    if (o.bound_push < 0 || o.bound_frac < 0 || o.mult_bound_push < 0)
        return fail(LAFSE3_EINVAL, "lafse3_ocp_solve_warm: negative push");
    lafse3::ExtArgs Z = {};
    Z.weights = weights;
    Z.rec = rec_out;
    lafse3::WarmArgs W = {};
    W.rec_in = rec_in;
    W.warm_out = warm_status;
    W.shift = o.shift < LAFSE3_MAX_N ? o.shift : LAFSE3_MAX_N;   // past the horizon every stage is the record's last
    W.mu_init = o.mu_init > 0 ? o.mu_init : c->prm.mu_init;
    W.bound_push = o.bound_push; W.bound_frac = o.bound_frac; W.mult_bound_push = o.mult_bound_push;
    return solve(c, B, ini, goal, p_tra, a_tra, t, u_last, x, u, lam, cost, status, iters, stream, &Z, &W);
}

// Not a solver launch (as trajectory scoring in launch()): its queue head is word 3 of the scoring counter block, and
// the solver block, the timing events and the error word of the last solver launch are left alone.
int lafse3_ocp_vjp(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *p_tra,
                   const double *a_tra, const double *t, const double *u_last, const double *weights,
                   const double *rec, const double *g_x, const double *g_u, int32_t groups, double *grad,
                   int32_t *sens_status, void *stream)
{
    if (!c) return fail(LAFSE3_EINVAL, "bad ctx / batch");
    if (groups == 0 || (groups & ~lafse3::SENS_W_ALL))
        return fail(LAFSE3_EINVAL, "lafse3_ocp_vjp: groups must be a non-empty subset of "
                                   "LAFSE3_SENS_THETA | LAFSE3_SENS_INI | LAFSE3_SENS_GOAL | LAFSE3_SENS_WEIGHTS");
    if (!rec || !grad) return fail(LAFSE3_EINVAL, "lafse3_ocp_vjp: rec and grad are required");
    if (const int rc = check_call(c, B, {ini, goal, p_tra, a_tra, t})) return rc;
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    const int64_t grid = B < c->slots ? B : c->slots;
    if (const int rc = reserve_ws(c, grid)) return rc;
    lafse3::VjpArgs A;
    std::memset(&A, 0, sizeof(A));
    A.prm = c->prm;
    A.n_inst = B;
    A.goal = goal; A.ptra = p_tra; A.atra = a_tra; A.t = t; A.ulast = u_last;   // ini_state: stage 0 of the record
    A.weights = weights;
    A.rec = rec; A.gx = g_x; A.gu = g_u;
    A.grad = grad; A.sens_out = sens_status; A.groups = groups;
    A.counters = c->counters.data() + N_COUNTERS;
    A.ws = c->ws.data();
    hipStream_t st = (hipStream_t)stream;
    // the queue head alone: the kernel touches no other word of the block
    hipError_t e = hipMemsetAsync(A.counters + 3, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemsetAsync", e);
    hipLaunchKernelGGL(lafse3::vjp_kernel, dim3((unsigned)grid), dim3(64), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "vjp kernel launch", e);
    return LAFSE3_OK;
}

// ---- fp32 twin of lafse3_ocp_solve: float inputs/outputs at the boundary, fp64 arithmetic inside (IPOPT's
// 1e-8 tolerance is below float32 resolution, so the solve itself cannot run in fp32)
__global__ void f32_to_f64_kernel(const float *in, double *out, int64_t n)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < n) out[e] = (double)in[e];
}

__global__ void f64_to_f32_kernel(const double *in, float *out, int64_t n)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < n) out[e] = (float)in[e];
}

static int convert(const void *in, void *out, int64_t n, bool to64, hipStream_t st)
{
    if (n == 0 || !in || !out) return LAFSE3_OK;
    const char *what = "fp32/fp64 conversion launch";
    if (to64) return launch_flat(f32_to_f64_kernel, n, st, what, (const float *)in, (double *)out, n);
    return launch_flat(f64_to_f32_kernel, n, st, what, (const double *)in, (float *)out, n);
}

int lafse3_ocp_solve_f32(lafse3_ctx *c, int64_t B, const float *ini, const float *goal, const float *p_tra,
                         const float *a_tra, const float *t, const float *u_last, float *x, float *u, float *lam,
                         float *cost, int32_t *status, int32_t *iters, void *stream)
{
    if (const int rc = check_call(c, B, {ini, goal, p_tra, a_tra, t})) return rc;
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    const int64_t N = c->prm.horizon;
    const int64_t nin = B * (13 + 3 + 3 + 3 + 1 + 4);
    const int64_t nx = x ? B * (N + 1) * 13 : 0, nu = u ? B * N * 4 : 0, nl = lam ? B * N * 13 : 0, nc = cost ? B : 0;
    const int64_t need = nin + nx + nu + nl + nc;
    const hipError_t e = c->tmp32.ensure(need);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMalloc fp32 staging", e);
    double *d = c->tmp32.data();
    double *dini = d, *dgoal = dini + 13 * B, *dp = dgoal + 3 * B, *da = dp + 3 * B, *dt = da + 3 * B, *dul = dt + B;
    double *dx = dul + 4 * B, *du = dx + nx, *dl = du + nu, *dc = dl + nl;
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    if ((rc = convert(ini, dini, 13 * B, true, st)) || (rc = convert(goal, dgoal, 3 * B, true, st)) ||
        (rc = convert(p_tra, dp, 3 * B, true, st)) || (rc = convert(a_tra, da, 3 * B, true, st)) ||
        (rc = convert(t, dt, B, true, st)) || (rc = convert(u_last, dul, u_last ? 4 * B : 0, true, st)))
        return rc;
    rc = lafse3_ocp_solve(c, B, dini, dgoal, dp, da, dt, u_last ? dul : nullptr, x ? dx : nullptr, u ? du : nullptr,
                          lam ? dl : nullptr, cost ? dc : nullptr, status, iters, stream);
    if (rc) return rc;
    if ((rc = convert(dx, x, nx, false, st)) || (rc = convert(du, u, nu, false, st)) ||
        (rc = convert(dl, lam, nl, false, st)) || (rc = convert(dc, cost, nc, false, st)))
        return rc;
    return LAFSE3_OK;
}

int lafse3_objective(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *gate12,
                     const double *p_tra, const double *a_tra, const double *t, const double *u_last, double *reward,
                     int32_t *status, void *stream)
{
    if (const int rc = check_call(c, B, {ini, goal, gate12, p_tra, a_tra, t, reward})) return rc;
    if (const int rc = check_reward_horizon(c, "lafse3_objective")) return rc;
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    lafse3::KernelArgs A = blank_args();
    A.mode = lafse3::MODE_OBJECTIVE;
    A.n_inst = B;
    A.ini = ini; A.goal = goal; A.gate12 = gate12; A.ptra = p_tra; A.atra = a_tra; A.t = t; A.ulast = u_last;
    A.reward_out = reward; A.status_out = status;
    return launch(c, A, (hipStream_t)stream);
}

int lafse3_sol_gradient(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *gate12,
                        const float *dnn_out, const double *u_last, double *out8, double *rewards9, int32_t *status9,
                        void *stream)
{
    if (const int rc = check_call(c, B, {ini, goal, gate12, dnn_out, out8}, 9)) return rc;
    if (const int rc = check_reward_horizon(c, "lafse3_sol_gradient")) return rc;
    const bool ift = c->prm.grad_mode == 1;
    if (ift && u_last) return fail(LAFSE3_EINVAL, "grad_mode 1 (IFT) linearises the nominal solve: u_last must be NULL");
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    double *R = rewards9;
    if (!R) {
        const hipError_t e = c->tmp.ensure(B * 9);
        if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMalloc scratch", e);
        R = c->tmp.data();
    }
    lafse3::KernelArgs A = blank_args();
    A.mode = lafse3::MODE_GRAD;
    A.n_inst = ift ? B * 3 : B * 9;   // IFT: nominal + the two t probes; slots of rewards9 / status9 unchanged
    A.ini = ini; A.goal = goal; A.gate12 = gate12; A.dnn = dnn_out; A.ulast = u_last;
    A.reward_out = R; A.status_out = status9;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_flat(slots_init_kernel, 9 * B, st, "slots_init_kernel launch", R, status9, 9 * B);
    if (rc) return rc;
    rc = launch(c, A, st, B);   // nominal solves first, then the probes longest-first (sched_next)
    if (rc) return rc;
    return launch_flat(lafse3::assemble_kernel, B, st, "assemble_kernel launch", B, R, dnn_out, out8);
}

int lafse3_get_input(lafse3_ctx *c, int64_t B, const double *ini, const double *goal, const double *u_last,
                     const float *dnn_out, double *u0, double *x, int32_t *status, void *stream)
{
    if (const int rc = check_call(c, B, {ini, goal, dnn_out, u0})) return rc;
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    const int N = c->prm.horizon;
    // full control trajectory goes to scratch; u0 is its first row (copied with a 2-D memcpy)
    hipError_t e = c->tmp.ensure(B * (int64_t)N * 4);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMalloc scratch", e);
    lafse3::KernelArgs A = blank_args();
    A.mode = lafse3::MODE_GETINPUT;
    A.n_inst = B;
    A.ini = ini; A.goal = goal; A.dnn = dnn_out; A.ulast = u_last;
    A.u_out = c->tmp.data(); A.x_out = x; A.status_out = status;
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch(c, A, st);
    if (rc) return rc;
    e = hipMemcpy2DAsync(u0, 4 * sizeof(double), c->tmp.data(), (size_t)N * 4 * sizeof(double), 4 * sizeof(double),
                         (size_t)B, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemcpy2DAsync", e);
    return LAFSE3_OK;
}

int lafse3_reward(lafse3_ctx *c, int64_t B, const double *x, const double *goal, const double *gate12, double *reward,
                  void *stream)
{
    if (const int rc = check_call(c, B, {x, goal, gate12, reward})) return rc;
    if (const int rc = check_reward_horizon(c, "lafse3_reward")) return rc;
    if (B == 0) return LAFSE3_OK;
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    lafse3::KernelArgs A = blank_args();
    A.mode = lafse3::MODE_REWARD;
    A.n_inst = B;
    A.x_in = x; A.goal = goal; A.gate12 = gate12; A.reward_out = reward;
    // the same persistent launch as the solves: min(B, slots) workgroups, each with its own workspace slot
    return launch(c, A, (hipStream_t)stream);
}

int lafse3_traversal_time(lafse3_ctx *c, int64_t B, const double *state, const double *final_point,
                          const double *gate12, const double *velo, double w, const float *dnn2_weights,
                          double *t_out, int32_t *iters, void *stream)
{
    if (const int rc = check_call(c, B, {state, final_point, gate12, velo, dnn2_weights, t_out})) return rc;
    if (B == 0) return LAFSE3_OK;
    if (((uintptr_t)dnn2_weights & 15) != 0) return fail(LAFSE3_EINVAL, "dnn2_weights not 16-byte aligned");
    DeviceGuard dev(c->device);
    if (dev.err != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", dev.err);
    lafse3::TTArgs A;
    A.B = B;
    A.state = state; A.final_point = final_point; A.gate = gate12; A.velo = velo;
    A.w = w;
    A.weights = dnn2_weights;
    A.t_out = t_out;
    A.iters = iters;
    // one wave per episode, grid-stride: two rounds of resident waves (1 per SIMD at its register count)
    const int64_t grid = B < 2 * c->slots ? B : 2 * c->slots;
    hipLaunchKernelGGL(lafse3::traversal_time_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "traversal_time launch", e);
    return LAFSE3_OK;
}

int lafse3_dnn2_weight_count(void) { return lafse3::TT_NW; }

float lafse3_last_kernel_ms(const lafse3_ctx *c)
{
    if (!c || !c->timed) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0f;
    return ms;
}

// The three counter readers open alike: arguments, then a context with no solver launch yet (which
// lafse3_check_device passes as clean, idle_ok, and the other two refuse), then the read into h.  LAFSE3_EINVAL
// means that nothing was read.
static int read_counters(lafse3_ctx *c, const void *out, bool idle_ok, unsigned long long (&h)[N_COUNTERS])
{
    if (!c || !out) return fail(LAFSE3_EINVAL, "null argument");
    if (!c->timed) return idle_ok ? LAFSE3_OK : fail(LAFSE3_EINVAL, "no solver launch on this context yet");
    // the counters are written by the last solver launch: wait for its end event (recorded on the launch stream,
    // which may be a non-blocking torch stream or one the caller has destroyed since), then copy on the context's
    // own stream -- not on the launch stream and not on the legacy default stream
    DeviceGuard dev(c->device);
    hipError_t e = dev.err;
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipSetDevice", e);
    e = hipEventSynchronize(c->ev1);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h, c->counters.data(), sizeof(h), hipMemcpyDeviceToHost, c->aux);
    if (e == hipSuccess) e = hipStreamSynchronize(c->aux);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemcpyAsync counters", e);
    if (h[lafse3::CNT_ERR]) {
        char buf[200];
        snprintf(buf, sizeof(buf), "device error word 0x%llx raised by a solver launch since the last lafse3_check_device%s",
                 h[lafse3::CNT_ERR],
                 (h[lafse3::CNT_ERR] & lafse3::ERR_PROBE_LOST)
                     ? ": a sol_gradient probe task was lost (its rewards9/status9 slot holds NaN / status 7)" : "");
        return fail(LAFSE3_EDEVICE, buf);
    }
    return LAFSE3_OK;
}

int lafse3_last_counters(lafse3_ctx *c, int64_t counters[3])
{
    unsigned long long h[N_COUNTERS] = {};
    const int rc = read_counters(c, counters, false, h);
    if (rc == LAFSE3_EINVAL) return rc;
    for (int i = 0; i < 3; ++i) counters[i] = (int64_t)h[i];
    return rc;
}

int lafse3_last_resto_counters(lafse3_ctx *c, int64_t counters[2])
{
    unsigned long long h[N_COUNTERS] = {};
    const int rc = read_counters(c, counters, false, h);
    if (rc == LAFSE3_EINVAL) return rc;
    counters[0] = (int64_t)h[lafse3::CNT_RESTO];
    counters[1] = (int64_t)h[lafse3::CNT_RESTO + 1];
    return rc;
}

int lafse3_check_device(lafse3_ctx *c)
{
    unsigned long long h[N_COUNTERS] = {};
    const int rc = read_counters(c, c, true, h);
    if (!h[lafse3::CNT_ERR]) return rc;   // clean, nothing to read yet, or the read itself failed
    // reported: clear it for the launches that follow
    DeviceGuard dev(c->device);
    hipError_t e = dev.err;
    if (e == hipSuccess)
        e = hipMemsetAsync(c->counters.data() + lafse3::CNT_ERR, 0, sizeof(unsigned long long), c->aux);
    if (e == hipSuccess) e = hipStreamSynchronize(c->aux);
    if (e != hipSuccess) return fail(LAFSE3_EDEVICE, "hipMemsetAsync error word", e);
    return rc;
}

int lafse3_debug_drop_push(lafse3_ctx *c, int64_t sample)
{
    if (!c) return fail(LAFSE3_EINVAL, "null ctx");
    c->drop_push = sample;
    return LAFSE3_OK;
}

int lafse3_debug_trace(lafse3_ctx *c, double *buf, int iters)
{
    if (!c) return fail(LAFSE3_EINVAL, "null ctx");
    c->trace = buf;
    c->trace_iters = buf ? iters : 0;
    return LAFSE3_OK;
}

int lafse3_debug_timers(lafse3_ctx *c, uint64_t *buf)
{
    if (!c) return fail(LAFSE3_EINVAL, "null ctx");
    c->ptime = (unsigned long long *)buf;
    return LAFSE3_OK;
}

int lafse3_debug_dump(lafse3_ctx *c, double *buf, int it, int after_refine)
{
    if (!c) return fail(LAFSE3_EINVAL, "null ctx");
    c->dump = buf;
    c->dump_it = buf ? it : -1;
    c->dump_refine = after_refine;
    return LAFSE3_OK;
}

int lafse3_debug_dump_resto(lafse3_ctx *c, double *buf, int entry, int it, int after_refine)
{
    if (!c) return fail(LAFSE3_EINVAL, "null ctx");
    if (buf && (entry < 0 || it < 0)) return fail(LAFSE3_EINVAL, "debug_dump_resto: entry and it must be >= 0");
    c->rdump.buf = buf;
    c->rdump.entry = buf ? entry : -1;
    c->rdump.it = buf ? it : -1;
    c->rdump.refine = after_refine ? 1 : 0;
    return LAFSE3_OK;
}

int lafse3_record_iters(lafse3_ctx *c, int32_t *buf, int64_t capacity)
{
    if (!c) return fail(LAFSE3_EINVAL, "null ctx");
    if (buf && capacity <= 0) return fail(LAFSE3_EINVAL, "record_iters: capacity must be > 0");
    c->iters_rec = buf;
    c->iters_cap = buf ? capacity : 0;
    return LAFSE3_OK;
}

const char *lafse3_last_error(void) { return g_err.c_str(); }

const char *lafse3_version(void) { return "lafse3 0.7.0 (gfx950)"; }

}  // extern "C"
