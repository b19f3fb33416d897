// User-supplied ODE right-hand sides: hiprtc builds of the forward / interrogation kernels.
//
// rodeo's `ode_fun` is an arbitrary Python callable evaluated inside the scan (src/rodeo/solve.py:70-78) and
// differentiated by jax.jacfwd (src/rodeo/interrogate.py:76).  Here the time loop lives in one GPU kernel, so a new ODE
// arrives as HIP source for a small struct (the interface of csrc/rhs.hpp, or a scalar-generic `rhs` wrapped by
// rk::AutoJac of csrc/dual.hpp for the Jacobian) and the kernel templates are instantiated for it at run time, once per
// JitKey actually used.  The observation models of DALTON's non-Gaussian form (rodeo_amd.trace.trace_obs_source) arrive the
// same way; their kernels are built around EITHER kind of right-hand side, a built-in one named through the embedded rhs.hpp.
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <link.h>
#include <limits.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <optional>
#include <string>
#include <tuple>
#include <vector>
#include "common.hpp"
#include "solve_args.hpp"
#include "solve_dense_itg_kernels.hpp"
#include "solve_paths.hpp"
#include "daltonng_kernels.hpp"
#include "build/embedded_sources.inc"

namespace rk {

struct UserRhs {
    std::string type_name;      // C++ type inside namespace rk, e.g. "MyOde" or "AutoJac<MyOde>"
    std::string source;
    int n_block, n_theta, n_bmeas;
};

struct UserObs {
    std::string type_name, source;
    int n_block, n_bstate, n_ycols, n_theta, n_active;
};

// The registries and the two caches below share one mutex.  It is never held through a hiprtc build (jit_lookup).
static std::mutex g_mu;
static std::deque<UserRhs> g_rhs;                                    // id = RK_RHS_USER_BASE + index; entries never move or change
static std::deque<UserObs> g_obs;                                    // id = index; likewise

// One row per JitKind.  expr: the kernel's name expression, with {P} = n_bstate, {I} = interrogate, {M} = n_bobs, {NB} = the
// blocked tile kernel's instance, {A} = the observation model's n_active; rk::UserRhsT / rk::UserObsT alias the user's types
// inside the translation unit (they may be template-ids).  header: included by this kind only, so that the program text of
// every other build stays what it was.  label: the launch's name in the profile (none: not bracketed).
struct JitKindRow { const char *expr, *header, *label; };
static const JitKindRow kJitKinds[JIT_N_KINDS] = {
    /* JIT_FWD                */ {"rk::fwd_kernel<rk::UserRhsT, {P}, {I}, false>", nullptr, "fwd_kernel<user>"},
    /* JIT_FWD_STORE_PRED     */ {"rk::fwd_kernel<rk::UserRhsT, {P}, {I}, true>", nullptr, "fwd_kernel<user>"},
    /* JIT_ITG                */ {"rk::interrogate_kernel<rk::UserRhsT, {P}, {I}>", nullptr, nullptr},
    /* JIT_TILE3              */ {"rk::fwd_tile3_kernel<rk::UserRhsT, {I}>", nullptr, "fwd_tile3_kernel<user>"},
    /* JIT_TILE4              */ {"rk::fwd_tile4_kernel<rk::UserRhsT, {I}>", nullptr, "fwd_tile4_kernel<user>"},
    /* JIT_TILEN              */ {"rk::fwd_tilen_kernel<rk::UserRhsT, {I}, {NB}>", nullptr, "fwd_tilen_kernel<user>"},
    /* JIT_SQRT               */ {"rk::fwd_sqrt_kernel<rk::UserRhsT, {P}, {I}>", nullptr, "fwd_sqrt_kernel<user>"},
    /* JIT_FWD_M              */ {"rk::fwd_kernel_m<rk::UserRhsT, {P}, {I}, false>", nullptr, "fwd_kernel<user>"},
    /* JIT_FWD_M_STORE_PRED   */ {"rk::fwd_kernel_m<rk::UserRhsT, {P}, {I}, true>", nullptr, "fwd_kernel<user>"},
    /* JIT_DENSE_ITG          */ {"rk::dense_interrogate_kernel<rk::UserRhsT::Inner, {P}, {I}>", nullptr, nullptr},
    /* JIT_ITG_M              */ {"rk::interrogate_kernel_m<rk::UserRhsT, {P}, {I}>", nullptr, nullptr},
    /* JIT_DALTON             */ {"rk::dalton_fwd_kernel<rk::UserRhsT, {P}, {I}, {M}, false>", "dalton_kernels.hpp", "dalton_fwd_kernel<loglik, user>"},
    /* JIT_DALTON_STORE       */ {"rk::dalton_fwd_kernel<rk::UserRhsT, {P}, {I}, {M}, true>", "dalton_kernels.hpp", "dalton_fwd_kernel<store, user>"},
    /* JIT_DALTON_TILE3       */ {"rk::dalton_fwd_tile3_kernel<rk::UserRhsT, {I}, false>", "dalton_tile3_kernels.hpp", "dalton_fwd_tile3_kernel<loglik, user>"},
    /* JIT_DALTON_TILE3_STORE */ {"rk::dalton_fwd_tile3_kernel<rk::UserRhsT, {I}, true>", "dalton_tile3_kernels.hpp", "dalton_fwd_tile3_kernel<store, user>"},
    /* JIT_DALTONNG           */ {"rk::daltonng_fwd_kernel<rk::UserRhsT, rk::UserObsT, {P}, {I}, {A}, false>", "daltonng_kernels.hpp", "daltonng_fwd_kernel<store>"},
    /* JIT_DALTONNG_BOTH      */ {"rk::daltonng_fwd_kernel<rk::UserRhsT, rk::UserObsT, {P}, {I}, {A}, true>", "daltonng_kernels.hpp", "daltonng_fwd_kernel<both>"},
    /* JIT_DALTONNG_OBS       */ {"rk::daltonng_obs_kernel<rk::UserObsT>", "daltonng_kernels.hpp", "daltonng_obs_kernel"},
    /* JIT_DALTON_AT          */ {"rk::dalton_fwd_at_kernel<rk::UserRhsT, {P}, {I}, {M}>", "dalton_at_kernels.hpp", "dalton_fwd_at_kernel<user>"},
    /* JIT_DALTON_AT_TILE3    */ {"rk::dalton_fwd_at_tile3_kernel<rk::UserRhsT, {I}>", "dalton_at_tile3_kernels.hpp", "dalton_fwd_at_tile3_kernel<user>"},
    /* JIT_EVIDENCE           */ {"rk::evidence_kernel<rk::UserRhsT, {P}, {I}>", "evidence_kernels.hpp", "evidence_kernel<user>"},
    /* JIT_EVIDENCE_TILE3     */ {"rk::evidence_tile3_kernel<rk::UserRhsT, {I}>", "evidence_tile3_kernels.hpp", "evidence_tile3_kernel<user>"},
    /* JIT_EVIDENCE_SQRT      */ {"rk::evidence_sqrt_kernel<rk::UserRhsT, {P}, {I}>", "evidence_kernels.hpp", "evidence_sqrt_kernel<user>"},
    /* JIT_DYNAMIC            */ {"rk::dynamic_fwd_kernel<rk::UserRhsT, {P}, {I}>", "dynamic_kernels.hpp", "dynamic_fwd_kernel<user>"},
    /* JIT_GRID               */ {"rk::grid_fwd_kernel<rk::UserRhsT, {P}, {I}>", "grid_kernels.hpp", "grid_fwd_kernel<user>"},
    /* JIT_DALTON_GRID        */ {"rk::dalton_grid_fwd_kernel<rk::UserRhsT, {P}, {I}, {M}, false>", "dalton_grid_kernels.hpp", "dalton_grid_fwd_kernel<loglik, user>"},
    /* JIT_DALTON_GRID_STORE  */ {"rk::dalton_grid_fwd_kernel<rk::UserRhsT, {P}, {I}, {M}, true>", "dalton_grid_kernels.hpp", "dalton_grid_fwd_kernel<store, user>"},
    /* JIT_GRID_EVIDENCE      */ {"rk::grid_evidence_kernel<rk::UserRhsT, {P}, {I}>", "grid_calib_kernels.hpp", "grid_evidence_kernel<user>"},
    /* JIT_GRID_DYNAMIC       */ {"rk::grid_dynamic_fwd_kernel<rk::UserRhsT, {P}, {I}>", "grid_calib_kernels.hpp", "grid_dynamic_fwd_kernel<user>"},
    /* JIT_DALTONNG_GRID      */ {"rk::daltonng_grid_fwd_kernel<rk::UserRhsT, rk::UserObsT, {P}, {I}, {A}, false>", "daltonng_grid_kernels.hpp", "daltonng_grid_fwd_kernel<store>"},
    /* JIT_DALTONNG_GRID_BOTH */ {"rk::daltonng_grid_fwd_kernel<rk::UserRhsT, rk::UserObsT, {P}, {I}, {A}, true>", "daltonng_grid_kernels.hpp", "daltonng_grid_fwd_kernel<both>"},
    /* JIT_DALTON_GRAD        */ {"rk::dalton_grid_jvp_kernel<rk::UserRhsT, {P}, {I}>", "dalton_grad_kernels.hpp", "dalton_grid_jvp_kernel<user>"},
    /* JIT_FENRIR_GRAD        */ {"rk::fenrir_grid_jvp_fwd_kernel<rk::UserRhsT, {P}, {I}>", "fenrir_grad_kernels.hpp", "fenrir_grid_jvp_fwd_kernel<user>"},
    /* JIT_DALTON_GRAD_HYPER  */ {"rk::dalton_grid_jvp_hyper_kernel<rk::UserRhsT, {P}, {I}>", "dalton_grad_kernels.hpp", "dalton_grid_jvp_hyper_kernel<user>"},
    /* JIT_FENRIR_GRAD_HYPER  */ {"rk::fenrir_grid_jvp_fwd_hyper_kernel<rk::UserRhsT, {P}, {I}>", "fenrir_grad_kernels.hpp", "fenrir_grid_jvp_fwd_hyper_kernel<user>"},
};

// What one build depends on.  A field that the kind's name expression does not read stays 0 (obs: -1, no observation
// model), so that configurations which share a kernel share its build.  device: -1 in the code map.
struct JitKey {
    int rhs, obs, n_bstate, n_bobs, nb, interrogate;
    JitKind kind;
    int device;
    bool operator<(const JitKey& o) const {
        return std::tie(rhs, obs, n_bstate, n_bobs, nb, interrogate, kind, device) <
               std::tie(o.rhs, o.obs, o.n_bstate, o.n_bobs, o.nb, o.interrogate, o.kind, o.device);
    }
};

// the key of `kind` for a configuration: which fields count is read off the kind's name expression
static JitKey jit_key(JitKind kind, int rhs_id, const rk_solve_cfg* c, int n_bobs = 0, int obs_id = -1) {
    const auto reads = [&](const char* tag) { return strstr(kJitKinds[kind].expr, tag) != nullptr; };
    JitKey k;
    k.rhs = reads("UserRhsT") ? rhs_id : 0;
    k.obs = reads("UserObsT") ? obs_id : -1;
    k.n_bstate = reads("{P}") ? c->n_bstate : 0;
    k.n_bobs = reads("{M}") ? n_bobs : 0;
    k.nb = reads("{NB}") ? (c->n_bstate <= 4 ? 1 : 2) : 0;             // solve_tilen_kernels.hpp: NB = 1 (p = 4) / 2 (p = 5 .. 8)
    k.interrogate = reads("{I}") ? c->interrogate : 0;
    k.kind = kind;
    k.device = -1;
    return k;
}

static std::string kernel_expr(const JitKey& k, int n_active) {
    std::string s = kJitKinds[k.kind].expr;
    const std::pair<const char*, int> fields[] = {{"{P}", k.n_bstate}, {"{I}", k.interrogate}, {"{M}", k.n_bobs},
                                                  {"{NB}", k.nb}, {"{A}", n_active}};
    for (const auto& f : fields)
        for (size_t at; (at = s.find(f.first)) != std::string::npos;) s.replace(at, strlen(f.first), std::to_string(f.second));
    return s;
}

// Are BOTH the libhiprtc behind hiprtcCompileProgram and the compiler library it drives (libamd_comgr) the ones under
// /opt/rocm (the toolchain of this build)?  Evaluated at the first compilation, i.e. after whatever the process has loaded
// by then: torch imported BEFORE this library brings its own libhiprtc, torch imported AFTER it (but before the first
// build) its own libamd_comgr, which the system's hiprtc then picks up -- either way the option must stay away.
// RK_JIT_BACKEND_OPTIONS = 0 / 1 overrides.
static bool under_opt_rocm(const char* path) {
    char real[PATH_MAX];
    const char* r = path && realpath(path, real) ? real : path;
    return r && strncmp(r, "/opt/rocm", 9) == 0;
}
static int find_comgr(struct dl_phdr_info* info, size_t, void* out) {
    if (info->dlpi_name && strstr(info->dlpi_name, "libamd_comgr")) {
        *(std::string*)out = info->dlpi_name;
        return 1;
    }
    return 0;
}
static bool hiprtc_takes_backend_options() {
    static const int v = [] {
        if (const char* e = getenv("RK_JIT_BACKEND_OPTIONS")) return atoi(e) != 0 ? 1 : 0;
        Dl_info info;
        if (!dladdr((void*)&hiprtcCompileProgram, &info) || !under_opt_rocm(info.dli_fname)) return 0;
        std::string comgr;
        dl_iterate_phdr(find_comgr, &comgr);
        if (comgr.empty()) {                              // not loaded yet: take the one next to this hiprtc, now
            std::string dir(info.dli_fname);
            dir.erase(dir.find_last_of('/') + 1);
            if (!dlopen((dir + "libamd_comgr.so.3").c_str(), RTLD_NOW | RTLD_GLOBAL)) return 0;
            dl_iterate_phdr(find_comgr, &comgr);
        }
        return !comgr.empty() && under_opt_rocm(comgr.c_str()) ? 1 : 0;
    }();
    return v != 0;
}

// one hiprtc build of `src` for the kernel named by `expr`: the code object in `code`, the mangled name in `lowered`; `role` and
// `what` name the user's code in the error message
static int jit_compile_src(const std::string& src, const std::string& expr, const std::string& what, std::vector<char>& code,
                           std::string& lowered, const char* role) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "rk_user_rhs.hip", kJitNumHeaders, kJitHeaderSources, kJitHeaderNames) !=
        HIPRTC_SUCCESS) {
        set_error("hiprtcCreateProgram failed");
        return RK_ERR_HIP;
    }
    hiprtcAddNameExpression(prog, expr.c_str());
    // (Makefile: why aligned loops; MFMA results in VGPRs like the ahead-of-time build -- without it every MFMA result of the
    // tile kernels goes through an AGPR and two v_accvgpr_read, 12 extra instructions per step of the p = 3 forward kernel:
    // 0.79 against 0.67 ms on the headline shape.)  The -mllvm option exists in the ROCm compiler this library was built
    // with; an unknown -mllvm option makes LLVM call exit(), and in a process that loaded another ROCm first (import torch:
    // its wheel carries its own libhiprtc / comgr under the same soname) the calls below land in THAT one -- so the
    // option is passed only when the hiprtc that serves us is the system's.
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-falign-loops=64", "-mllvm", "-amdgpu-mfma-vgpr-form"};
    const hiprtcResult r = hiprtcCompileProgram(prog, hiprtc_takes_backend_options() ? 6 : 4, opts);
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        if (log.size() > 800) log.resize(800);
        set_error("hiprtc could not compile the %s '%s': %s", role, what.c_str(), log.c_str());
        hiprtcDestroyProgram(&prog);
        return RK_ERR_INVALID;
    }
    const char* low = nullptr;
    if (hiprtcGetLoweredName(prog, expr.c_str(), &low) != HIPRTC_SUCCESS || !low) {
        set_error("hiprtcGetLoweredName failed for %s", expr.c_str());
        hiprtcDestroyProgram(&prog);
        return RK_ERR_HIP;
    }
    lowered = low;
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    code.resize(cs);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    return RK_OK;
}

// the registered right-hand side behind rhs_id, or the error (the entry is immutable: the pointer is good without the lock)
static int user_rhs(int rhs_id, const UserRhs** u) {
    std::lock_guard<std::mutex> lk(g_mu);
    const int idx = rhs_id - RK_RHS_USER_BASE;
    RK_REQUIRE(idx >= 0 && idx < (int)g_rhs.size(), RK_ERR_INVALID, "unknown user rhs_id %d", rhs_id);
    *u = &g_rhs[idx];
    return RK_OK;
}
static int user_obs(int obs_id, const UserObs** u) {
    std::lock_guard<std::mutex> lk(g_mu);
    RK_REQUIRE(obs_id >= 0 && obs_id < (int)g_obs.size(), RK_ERR_INVALID, "unknown obs_id %d", obs_id);
    *u = &g_obs[obs_id];
    return RK_OK;
}

static const char* builtin_rhs_type(int rhs_id) {
    switch (rhs_id) {
        case RK_RHS_FITZHUGH_NAGUMO: return "FitzHughNagumo";
        case RK_RHS_LORENZ63: return "Lorenz63";
        case RK_RHS_HIGHER_ORDER: return "HigherOrder";
    }
    return nullptr;
}

// Compiled code objects, device independent, and the modules loaded from them per device.  A failed compilation is
// remembered with its message (the tile kernels are tried first and simply do not exist for some right-hand sides).
struct JitCode { int rc; std::vector<char> code; std::string lowered; std::string error; };
static std::map<JitKey, JitCode> g_code;                            // key.device = -1
static std::map<JitKey, hipFunction_t> g_mod;                       // key.device = the handle's

// RK_JIT_VERBOSE, at build time and without a device: the resources of the one kernel in a hiprtc code object, read from its
// AMDGPU metadata note (msgpack: the key's string, then an unsigned integer).  What the loaded kernel reports in jit_lookup, so
// that an instance's registers, scratch and LDS can be listed on a machine without a GPU.
static long jit_meta_uint(const std::vector<char>& code, const char* key) {
    const size_t n = strlen(key);
    for (size_t at = 0; at + n + 1 <= code.size(); ++at) {
        if (memcmp(code.data() + at, key, n) != 0) continue;
        const unsigned char* v = (const unsigned char*)code.data() + at + n;
        const size_t left = code.size() - (at + n);
        if (v[0] <= 0x7f) return v[0];
        if (v[0] == 0xcc && left >= 2) return v[1];
        if (v[0] == 0xcd && left >= 3) return (long)v[1] << 8 | v[2];
        if (v[0] == 0xce && left >= 5) return (long)v[1] << 24 | (long)v[2] << 16 | (long)v[3] << 8 | v[4];
    }
    return -1;
}
static void jit_report_build(const JitCode& b) {
    fprintf(stderr, "[rk] jit build %s: %ld VGPRs + %ld AGPRs, %ld B scratch per lane, %ld B LDS\n", b.lowered.c_str(),
            jit_meta_uint(b.code, ".vgpr_count"), jit_meta_uint(b.code, ".agpr_count"),
            jit_meta_uint(b.code, ".private_segment_fixed_size"), jit_meta_uint(b.code, ".group_segment_fixed_size"));
}

// program text, name expression and the user's type name (for the error message) of the build behind `key`
struct JitProgram { std::string src, expr, what; const char* role; };
static int jit_program(const JitKey& key, JitProgram& p) {
    const JitKindRow& row = kJitKinds[key.kind];
    const UserRhs* u = nullptr;
    const UserObs* ob = nullptr;
    int rc = is_user_rhs(key.rhs) ? user_rhs(key.rhs, &u) : RK_OK;
    if (rc == RK_OK && key.obs >= 0) rc = user_obs(key.obs, &ob);
    if (rc) return rc;
    // (neither: a built-in right-hand side under a kind that names one -- rk_fenrir_grad_compile_check's check of the header)
    const char* builtin = !u && !ob && strstr(row.expr, "UserRhsT") ? builtin_rhs_type(key.rhs) : nullptr;
    RK_REQUIRE(u || ob || builtin, RK_ERR_INVALID, "unknown user rhs_id %d", key.rhs);
    if (ob) p.src = std::string("#include \"solve_small_kernels.hpp\"\n#include \"dual.hpp\"\n") +
                    (u ? "" : "#include \"rhs.hpp\"\n");                // (a user's names stay free)
    else p.src = "#include \"solve_small_kernels.hpp\"\n#include \"dual.hpp\"\n"
                 "#include \"solve_tile3_kernels.hpp\"\n#include \"solve_tile4_kernels.hpp\"\n"
                 "#include \"solve_tilen_kernels.hpp\"\n#include \"solve_sqrt_kernels.hpp\"\n"
                 "#include \"solve_small_m_kernels.hpp\"\n#include \"solve_dense_itg_kernels.hpp\"\n";
    if (builtin) p.src += "#include \"rhs.hpp\"\n";
    if (row.header) p.src += std::string("#include \"") + row.header + "\"\n";
    p.src += "namespace rk {\n";
    if (u) {
        p.src += u->source + "\nusing UserRhsT = " + u->type_name + ";\n";
    } else if (strstr(row.expr, "UserRhsT")) {
        const char* t = builtin_rhs_type(key.rhs);
        RK_REQUIRE(t, RK_ERR_UNSUPPORTED, "daltonng: rhs %d has no lane-per-trajectory form", key.rhs);
        p.src += std::string("using UserRhsT = ") + t + ";\n";
    }
    if (ob) p.src += ob->source + "\nusing UserObsT = " + ob->type_name + ";\n";
    p.src += "}  // namespace rk\n";
    p.expr = kernel_expr(key, ob ? ob->n_active : 0);
    p.what = ob ? ob->type_name : u ? u->type_name : builtin;
    p.role = ob ? "observation log-likelihood" : u ? "user right-hand side" : "built-in right-hand side";
    return RK_OK;
}

// The one lookup: the build behind `key` (compiled once; a failure is remembered and returned with its message) and, with
// a handle, the kernel loaded on the handle's device.  g_mu is held for the map accesses and the module load only: the
// program text is put together from registry entries that never change, and hiprtc runs outside the lock -- a build takes
// seconds and must not hold up registrations or other handles.  Two threads that miss at once both compile; the first result
// inserted is kept.
static int jit_lookup(JitKey key, rk_handle h, hipFunction_t* fn) {
    const JitKey ckey = key;
    if (h) key.device = h->device;
    const JitCode* c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const auto mi = h ? g_mod.find(key) : g_mod.end();
        if (mi != g_mod.end()) { *fn = mi->second; return RK_OK; }
        const auto ci = g_code.find(ckey);
        if (ci != g_code.end()) c = &ci->second;
    }
    if (!c) {
        JitProgram p;
        const int rc = jit_program(ckey, p);
        if (rc) return rc;
        JitCode built;
        built.rc = jit_compile_src(p.src, p.expr, p.what, built.code, built.lowered, p.role);
        if (built.rc) built.error = rk_last_error();
        if (built.rc == RK_OK && getenv("RK_JIT_VERBOSE")) jit_report_build(built);
        std::lock_guard<std::mutex> lk(g_mu);
        c = &g_code.emplace(ckey, std::move(built)).first->second;     // (map nodes do not move: the pointer stays valid)
    }
    if (c->rc) { set_error("%s", c->error.c_str()); return c->rc; }
    if (!h) return RK_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    auto mi = g_mod.find(key);
    if (mi == g_mod.end()) {
        hipModule_t mod;
        hipFunction_t f;
        RK_HIP(hipModuleLoadData(&mod, c->code.data()));
        RK_HIP(hipModuleGetFunction(&f, mod, c->lowered.c_str()));
        if (getenv("RK_JIT_VERBOSE")) {                   // resources of the kernel hiprtc built (a spilled dual copy of a big system shows here)
            int regs = 0, scratch = 0, lds = 0;
            (void)hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, f);
            (void)hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f);
            (void)hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, f);
            fprintf(stderr, "[rk] jit kernel %s: %d registers, %d B scratch per lane, %d B LDS\n", c->lowered.c_str(), regs, scratch, lds);
        }
        mi = g_mod.emplace(key, f).first;
    }
    *fn = mi->second;
    return RK_OK;
}

// the kernel behind `key` on the handle's device, launched on the handle's stream under the kind's profile label
static int launch_jit(rk_handle h, const JitKey& key, LaunchGeom g, void** params) {
    hipFunction_t fn;
    const int rc = jit_lookup(key, h, &fn);
    if (rc) return rc;
    std::optional<LaunchTimer> t;
    if (kJitKinds[key.kind].label) t.emplace(h, kJitKinds[key.kind].label);
    RK_HIP(hipModuleLaunchKernel(fn, g.grid.x, 1, 1, g.block.x, 1, 1, 0, h->stream, params, nullptr));
    if (t) t->stop();
    return RK_OK;
}

bool is_user_rhs(int rhs_id) { return rhs_id >= RK_RHS_USER_BASE; }

// Does the MFMA-tile forward kernel exist for this user right-hand side and configuration?  (It needs NDEP == 1 and a
// block count the tile kernels support; decided by compiling it once -- cached -- so that rk_solve_layout and the
// solve agree.)  tile = JIT_TILE3 / JIT_TILE4 for n_bstate = 3 / 4, JIT_TILEN for the blocked tiles.
bool user_tile_available(const rk_solve_cfg* c, JitKind tile) {
    const UserRhs* u;
    if (user_rhs(c->rhs_id, &u)) return false;
    const int nb = u->n_block;
    if (c->n_block != nb || c->n_bmeas != 1 || u->n_bmeas != 1 || c->kalman_type != RK_KALMAN_STANDARD) return false;
    if (nb < 1 || nb > (tile == JIT_TILE4 ? 4 : 64)) return false;      // p = 3 and blocked tiles: up to 64 blocks (4 per wave, LDS exchange); p = 4: one wave
    const int rc = jit_lookup(jit_key(tile, c->rhs_id, c), nullptr, nullptr);
    if (rc && getenv("RK_JIT_VERBOSE")) fprintf(stderr, "[rk] tile kernel not available for user rhs %d (p = %d): %s\n", c->rhs_id, (int)tile, rk_last_error());
    return rc == RK_OK;
}

int user_forward_tile(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double* tiles, JitKind tile) {
    SolveArgs args = a;
    int P = c->n_bstate;
    void* params[] = {&args, &tiles, &P};                           // (the p = 3 / p = 4 kernels take the first two)
    const LaunchGeom g = fwd_tile_geom(a.B, c->n_block);
    launch_placement_primer(h, g.grid, g.block);
    return launch_jit(h, jit_key(tile, c->rhs_id, c), g, params);
}

int user_forward_sqrt(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a) {
    const int rc = user_lane_check(c, "square-root solver");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args};
    return launch_jit(h, jit_key(JIT_SQRT, c->rhs_id, c), fwd_sqrt_geom(a.B, c->n_block), params);
}

// Is the configuration the one rhs_id was registered for (n_block, n_bmeas), at an n_bstate the lane kernels serve?
int user_rhs_check(const rk_solve_cfg* c) {
    const UserRhs* u;
    const int rc = user_rhs(c->rhs_id, &u);
    if (rc) return rc;
    RK_REQUIRE(c->n_block == u->n_block && c->n_bmeas == u->n_bmeas, RK_ERR_UNSUPPORTED,
               "user rhs %d needs n_block=%d, n_bmeas=%d (got %d, %d)", c->rhs_id, u->n_block, u->n_bmeas, c->n_block, c->n_bmeas);
    const int pmax = c->n_bmeas > 1 ? 9 : 6;                     // (the backward kernels exist up to n_bstate = 9)
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= pmax, RK_ERR_UNSUPPORTED, "lane-per-trajectory path supports n_bstate in [2, %d] "
               "here, got %d", pmax, c->n_bstate);
    RK_REQUIRE(c->n_bmeas <= c->n_bstate, RK_ERR_INVALID, "n_bmeas = %d exceeds n_bstate = %d", c->n_bmeas, c->n_bstate);
    return RK_OK;
}

// ---- dense ("non-block") path: the interrogation kernel around the user's right-hand side (solve_dense_itg_kernels.hpp)
// Taken for one block with several measurements that the lane kernels do not serve (n_bstate > 9 or n_bmeas > 4).
static bool dense_wanted(const UserRhs& u, int n_bstate) { return u.n_block == 1 && u.n_bmeas > 1 && (n_bstate > 9 || u.n_bmeas > 4); }

bool user_dense_wanted(const rk_solve_cfg* c) {
    const UserRhs* u;
    return user_rhs(c->rhs_id, &u) == RK_OK && c->n_block == 1 && c->n_bmeas == u->n_bmeas && dense_wanted(*u, c->n_bstate);
}

int user_dense_interrogate(rk_handle h, const rk_solve_cfg* c, const DenseItgArgs& a) {
    DenseItgArgs args = a;
    void* params[] = {&args};
    return launch_jit(h, jit_key(JIT_DENSE_ITG, c->rhs_id, c), LaunchGeom{dim3(a.B), dim3(256)}, params);
}

int user_forward(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a) {
    const int rc = user_rhs_check(c);
    if (rc) return rc;
    const bool sp = (c->flags & RK_FLAG_STORE_PRED) != 0;
    const JitKind kind = c->n_bmeas > 1 ? (sp ? JIT_FWD_M_STORE_PRED : JIT_FWD_M) : (sp ? JIT_FWD_STORE_PRED : JIT_FWD);
    SolveArgs args = a;
    void* params[] = {&args};
    return launch_jit(h, jit_key(kind, c->rhs_id, c), fwd_lane_geom(a.B), params);
}

// DALTON's forward filters around a user right-hand side.  Lanes (dalton_kernels.hpp): the log-likelihood form (joint and
// marginal filter in the two halves of a wave) or the joint filter's store form.  Tiles (dalton_tile3_kernels.hpp,
// n_bstate = 3, n_bobs = 1): 2 B or B filter instances of n_block tiles.
int user_dalton(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, int n_bobs, bool store,
                bool tile, double* out) {
    const int rc = user_rhs_check(c);
    if (rc) return rc;
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "dalton: n_bmeas = 1 only");
    SolveArgs args = a;
    const DaltonObs* op = &o;
    void* params[] = {&args, (void*)op, &out};
    const JitKind kind = tile ? (store ? JIT_DALTON_TILE3_STORE : JIT_DALTON_TILE3) : (store ? JIT_DALTON_STORE : JIT_DALTON);
    return launch_jit(h, jit_key(kind, c->rhs_id, c, n_bobs), tile ? dalton_tile_geom(a.B, c->n_block, !store) : dalton_lane_geom(a.B, !store),
                      params);
}

// dalton_at's forward filters around a user right-hand side (dalton_at_kernels.hpp / dalton_at_tile3_kernels.hpp): the
// log-likelihood form only, launched like user_dalton's.
int user_dalton_at(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const DaltonAt& s, int n_bobs,
                   bool tile, double* out) {
    const int rc = user_rhs_check(c);
    if (rc) return rc;
    RK_REQUIRE(c->n_bmeas == 1, RK_ERR_UNSUPPORTED, "dalton_at: n_bmeas = 1 only");
    SolveArgs args = a;
    const DaltonObs* op = &o;
    const DaltonAt* sp = &s;
    void* params[] = {&args, (void*)op, (void*)sp, &out};
    return launch_jit(h, jit_key(tile ? JIT_DALTON_AT_TILE3 : JIT_DALTON_AT, c->rhs_id, c, n_bobs),
                      tile ? dalton_tile_geom(a.B, c->n_block, true) : dalton_lane_geom(a.B, true), params);
}

// The configuration against the registration for the lane families that keep their own n_bstate range (the square-root solver,
// solve_evidence, solve_mv_dynamic and every entry on the non-uniform grid): n_block and n_bmeas = 1 only.  `who` names the entry in the message.
// (user_rhs_check's bound of 6 is the standard lane kernels'; evidence's square-root lanes serve 2..8, like user_forward_sqrt.)
int user_lane_check(const rk_solve_cfg* c, const char* who) {
    const UserRhs* u;
    const int rc = user_rhs(c->rhs_id, &u);
    if (rc) return rc;
    RK_REQUIRE(c->n_block == u->n_block && c->n_bmeas == 1 && u->n_bmeas == 1, RK_ERR_UNSUPPORTED,
               "%s: user rhs %d needs n_block=%d, n_bmeas=1 (got %d, %d)", who, c->rhs_id, u->n_block, c->n_block, c->n_bmeas);
    return RK_OK;
}

// solve_evidence around a user right-hand side (evidence_tile3_kernels.hpp / evidence_kernels.hpp): the n_bstate range is
// evidence.hip's, per Kalman form.
// Does evidence_tile3_kernel exist for this user right-hand side (n_bstate = 3, standard form, up to four blocks, NDEP == 1)?
// Decided by building that kernel itself once (cached): the build that answers is the one the launch uses.
bool user_evidence_tile_available(const rk_solve_cfg* c) {
    if (user_lane_check(c, "evidence") || c->kalman_type != RK_KALMAN_STANDARD || c->n_bstate != 3 || c->n_block > 4) return false;
    const int rc = jit_lookup(jit_key(JIT_EVIDENCE_TILE3, c->rhs_id, c), nullptr, nullptr);
    if (rc && getenv("RK_JIT_VERBOSE")) fprintf(stderr, "[rk] evidence tile kernel not available for user rhs %d: %s\n", c->rhs_id, rk_last_error());
    return rc == RK_OK;
}

// the launch, like the built-in instances of evidence.hip; route: 0 tiles, 1 lanes, 2 square-root lanes
int user_evidence(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, int route, double* logdens, double* quad,
                  double* logdet) {
    const int rc = user_lane_check(c, "evidence");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args, &logdens, &quad, &logdet};
    const JitKind kind = route == 0 ? JIT_EVIDENCE_TILE3 : (route == 1 ? JIT_EVIDENCE : JIT_EVIDENCE_SQRT);
    const LaunchGeom g = route == 0 ? dalton_tile_geom(a.B, c->n_block, false)
                                    : (route == 1 ? fwd_lane_geom(a.B) : fwd_sqrt_geom(a.B, c->n_block));
    return launch_jit(h, jit_key(kind, c->rhs_id, c), g, params);
}

// solve_mv_dynamic / solve_sim_dynamic around a user right-hand side (dynamic_kernels.hpp): the configuration against the
// registration (n_block, n_bmeas = 1; the n_bstate range is dynamic.hip's) and the forward launch, like dynamic.hip's built-in
// instances.  The backward kernels do not depend on the right-hand side: dynamic.hip launches its own.
int user_dynamic(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double scale_min, double* scale, double* logdens) {
    const int rc = user_lane_check(c, "dynamic");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args, &scale_min, &scale, &logdens};
    return launch_jit(h, jit_key(JIT_DYNAMIC, c->rhs_id, c), fwd_lane_geom(a.B), params);
}

// solve_mv_grid / solve_sim_grid around a user right-hand side (grid_kernels.hpp): the configuration against the registration
// (n_block, n_bmeas = 1; the n_bstate range is grid.hip's) and the forward launch, like grid.hip's built-in instances.  The
// backward kernels do not depend on the right-hand side: grid.hip launches its own.
int user_grid(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g) {
    const int rc = user_lane_check(c, "grid");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args, (void*)&g};
    return launch_jit(h, jit_key(JIT_GRID, c->rhs_id, c), fwd_lane_geom(a.B), params);
}

// solve_evidence_grid / solve_mv_dynamic_grid / solve_sim_dynamic_grid around a user right-hand side (grid_calib_kernels.hpp):
// the configuration against the registration (n_block, n_bmeas = 1; the n_bstate ranges are grid_calib.hip's) and the forward
// launches, like grid_calib.hip's built-in instances.  The backward kernels do not depend on the right-hand side:
// grid_calib.hip launches its own.
int user_grid_evidence(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g, double* logdens, double* quad,
                       double* logdet) {
    const int rc = user_lane_check(c, "evidence_grid");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args, (void*)&g, &logdens, &quad, &logdet};
    return launch_jit(h, jit_key(JIT_GRID_EVIDENCE, c->rhs_id, c), fwd_lane_geom(a.B), params);
}

int user_grid_dynamic(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g, double scale_min, double* scale,
                      double* logdens) {
    const int rc = user_lane_check(c, "dynamic_grid");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args, (void*)&g, &scale_min, &scale, &logdens};
    return launch_jit(h, jit_key(JIT_GRID_DYNAMIC, c->rhs_id, c), fwd_lane_geom(a.B), params);
}

// dalton_grid around a user right-hand side (dalton_grid_kernels.hpp): the configuration against the registration (n_block,
// n_bmeas = 1; the n_bstate range is dalton_grid.hip's) and the forward launch, like dalton_grid.hip's built-in instances: the
// log-likelihood form (joint and marginal filter in the two halves of a wave) or the joint filter's store form.  The backward
// kernels do not depend on the right-hand side: grid.hip launches its own.
int user_dalton_grid(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& g, int n_bobs,
                     bool store, double* out) {
    const int rc = user_lane_check(c, "dalton_grid");
    if (rc) return rc;
    SolveArgs args = a;
    void* params[] = {&args, (void*)&o, (void*)&g, &out};
    return launch_jit(h, jit_key(store ? JIT_DALTON_GRID_STORE : JIT_DALTON_GRID, c->rhs_id, c, n_bobs), dalton_lane_geom(a.B, !store),
                      params);
}

// dalton_grid_jvp around a user right-hand side of the gradient kind (dalton_grad_kernels.hpp): the configuration against the
// registration (n_block, n_bmeas = 1) and the size limit of the built-in instances that ship (n_bstate 2 .. 3, n_block n_bstate^2
// <= 27: DESIGN.md section 7 (21)), then the launch, one (trajectory, direction) item per lane pair like dalton_grad.hip's.
int user_dalton_grad_check(const rk_solve_cfg* c) {
    const int rc = user_lane_check(c, "dalton_grid_jvp");
    if (rc) return rc;
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 3 && c->n_block * c->n_bstate * c->n_bstate <= 27, RK_ERR_UNSUPPORTED,
               "dalton_grid_jvp: not built: user rhs %d with %d blocks at n_bstate %d (n_bstate 2..3, n_block n_bstate^2 <= 27)",
               c->rhs_id, c->n_block, c->n_bstate);
    return RK_OK;
}

// (`hy`: null for the plain kernel, else the hyper kernel with its second struct of directions)
int user_dalton_grad(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const DaltonObs& o, const GridArgs& g, const JvpDirs& dir,
                     const JvpHyper* hy, int n_items, double* value, double* dvalue) {
    const int rc = user_dalton_grad_check(c);
    if (rc) return rc;
    SolveArgs args = a;
    void* plain[] = {&args, (void*)&o, (void*)&g, (void*)&dir, &value, &dvalue};
    void* hyper[] = {&args, (void*)&o, (void*)&g, (void*)&dir, (void*)hy, &value, &dvalue};
    return launch_jit(h, jit_key(hy ? JIT_DALTON_GRAD_HYPER : JIT_DALTON_GRAD, c->rhs_id, c), dalton_lane_geom(n_items, true),
                      hy ? hyper : plain);
}

// fenrir_grid_jvp's forward kernel around a user right-hand side of the gradient kind (fenrir_grad_kernels.hpp): dalton_grid_jvp's
// rule under this entry's name (n_block, n_bmeas = 1, n_bstate 2 .. 3, n_block n_bstate^2 <= 27: DESIGN.md section 7 (23)), then
// the launch, one (trajectory, direction) item per lane like fenrir_grad.hip's.
int user_fenrir_grad_check(const rk_solve_cfg* c) {
    const int rc = user_lane_check(c, "fenrir_grid_jvp");
    if (rc) return rc;
    RK_REQUIRE(c->n_bstate >= 2 && c->n_bstate <= 3 && c->n_block * c->n_bstate * c->n_bstate <= 27, RK_ERR_UNSUPPORTED,
               "fenrir_grid_jvp: not built: a user right-hand side with %d blocks at n_bstate %d (n_bstate 2 .. 3 and n_block "
               "n_bstate^2 <= 27)", c->n_block, c->n_bstate);
    return RK_OK;
}

int user_fenrir_grad(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, const GridArgs& g, const JvpDirs& dir, const JvpHyper* hy,
                     int n_items, double* dmean, double* dvar) {
    const int rc = user_fenrir_grad_check(c);
    if (rc) return rc;
    SolveArgs args = a;
    void* plain[] = {&args, (void*)&g, (void*)&dir, &dmean, &dvar};
    void* hyper[] = {&args, (void*)&g, (void*)&dir, (void*)hy, &dmean, &dvar};
    return launch_jit(h, jit_key(hy ? JIT_FENRIR_GRAD_HYPER : JIT_FENRIR_GRAD, c->rhs_id, c), dalton_lane_geom(n_items, false),
                      hy ? hyper : plain);
}

int user_interrogate(rk_handle h, const rk_solve_cfg* c, const SolveArgs& a, double t, int step, const double* mp,
                     const double* vp, double* wm, double* mm_, double* vm) {
    const int rc = user_rhs_check(c);
    if (rc) return rc;
    const bool multi = c->n_bmeas > 1;                     // several measurements per block: interrogate_kernel_m
    RK_REQUIRE(!multi || c->kalman_type == RK_KALMAN_STANDARD, RK_ERR_UNSUPPORTED,
               "rk_interrogate_batched: n_bmeas > 1 with kalman_type = square-root is fused into the solvers only");
    SolveArgs args = a;
    int sqrt_mode = c->kalman_type == RK_KALMAN_SQRT ? 1 : 0;
    void* params[] = {&args, &t, &step, &mp, &vp, &wm, &mm_, &vm, &sqrt_mode};
    return launch_jit(h, jit_key(multi ? JIT_ITG_M : JIT_ITG, c->rhs_id, c), fwd_lane_geom(a.B), params);
}

// ---- DALTON for non-Gaussian observations (daltonng_kernels.hpp): the observation log-likelihood is always user code, so
// its forward filter is a hiprtc build around either kind of right-hand side
int ng_obs_info(int obs_id, NgObsInfo* info) {
    const UserObs* u;
    const int rc = user_obs(obs_id, &u);
    if (rc) return rc;
    info->n_block = u->n_block; info->n_bstate = u->n_bstate; info->n_ycols = u->n_ycols; info->n_theta = u->n_theta;
    info->n_active = u->n_active;
    return RK_OK;
}

// the forward filter(s): joint moments into a.mean / a.var, with `both` the Z filter's into zm / zv
int ng_forward(rk_handle h, const rk_solve_cfg* c, int obs_id, const SolveArgs& a, const NgObs& o, bool both, double* zm,
               double* zv) {
    if (is_user_rhs(c->rhs_id)) {
        const int rc = user_rhs_check(c);
        if (rc) return rc;
    }
    SolveArgs args = a;
    NgObs obs = o;
    void* params[] = {&args, &obs, &zm, &zv};
    return launch_jit(h, jit_key(both ? JIT_DALTONNG_BOTH : JIT_DALTONNG, c->rhs_id, c, 0, obs_id), dalton_lane_geom(a.B, both), params);
}

// the same on rk_solve_grid's non-uniform grid (daltonng_grid_kernels.hpp): o.obs_ind holds the node of every observation
int ng_grid_forward(rk_handle h, const rk_solve_cfg* c, int obs_id, const SolveArgs& a, const NgObs& o, const GridArgs& g, bool both,
                    double* zm, double* zv) {
    if (is_user_rhs(c->rhs_id)) {
        const int rc = user_rhs_check(c);
        if (rc) return rc;
    }
    SolveArgs args = a;
    NgObs obs = o;
    void* params[] = {&args, &obs, (void*)&g, &zm, &zv};
    return launch_jit(h, jit_key(both ? JIT_DALTONNG_GRID_BOTH : JIT_DALTONNG_GRID, c->rhs_id, c, 0, obs_id),
                      dalton_lane_geom(a.B, both), params);
}

// logy_x on the smoothed means and the final sum into out (B)
int ng_obs_eval(rk_handle h, const rk_solve_cfg* c, int obs_id, const SolveArgs& a, const NgObs& o, const double* sm,
                const double* part, double* out) {
    int B = a.B, n_obs = o.n_obs, theta_b = a.theta_b;
    const double *y = o.y, *theta = a.theta;
    void* params[] = {&B, &n_obs, &y, &sm, &theta, &theta_b, &part, &out};
    return launch_jit(h, jit_key(JIT_DALTONNG_OBS, c->rhs_id, c, 0, obs_id), fwd_lane_geom(a.B), params);
}

}  // namespace rk

using namespace rk;

extern "C" {

int rk_register_rhs_source_m(const char* type_name, const char* source, int32_t n_block, int32_t n_bmeas, int32_t n_theta,
                             int32_t* rhs_id) {
    RK_REQUIRE(type_name && source && rhs_id, RK_ERR_INVALID, "rk_register_rhs_source: null argument");
    // (n_bmeas > 4: one block holding all variables, served by the dense path -- solve_dense.hip)
    RK_REQUIRE(n_block >= 1 && n_block <= 64 && n_theta >= 0 && n_bmeas >= 1 && (n_bmeas <= 4 || (n_block == 1 && n_bmeas <= 256)),
               RK_ERR_INVALID, "rk_register_rhs_source: bad n_block / n_bmeas / n_theta");
    std::lock_guard<std::mutex> lk(g_mu);
    g_rhs.push_back(UserRhs{type_name, source, n_block, n_theta, n_bmeas});
    *rhs_id = RK_RHS_USER_BASE + (int)g_rhs.size() - 1;
    return RK_OK;
}

int rk_register_rhs_source(const char* type_name, const char* source, int32_t n_block, int32_t n_theta, int32_t* rhs_id) {
    return rk_register_rhs_source_m(type_name, source, n_block, 1, n_theta, rhs_id);
}

int rk_register_obs_source(const char* type_name, const char* source, int32_t n_block, int32_t n_bstate, int32_t n_ycols,
                           int32_t n_theta, int32_t n_active, int32_t* obs_id) {
    RK_REQUIRE(type_name && source && obs_id, RK_ERR_INVALID, "rk_register_obs_source: null argument");
    RK_REQUIRE(n_block >= 1 && n_block <= 64 && n_bstate >= 2 && n_bstate <= 6 && n_ycols >= 1 && n_ycols <= 4 && n_theta >= 0 &&
               n_active >= 1 && n_active <= 3, RK_ERR_INVALID,
               "rk_register_obs_source: bad n_block / n_bstate (2..6) / n_ycols (1..4) / n_theta / n_active (1..3)");
    std::lock_guard<std::mutex> lk(g_mu);
    g_obs.push_back(UserObs{type_name, source, n_block, n_bstate, n_ycols, n_theta, n_active});
    *obs_id = (int)g_obs.size() - 1;
    return RK_OK;
}

int rk_obs_compile_check(int32_t obs_id, int32_t rhs_id, int32_t interrogate) {
    NgObsInfo info;
    int rc = ng_obs_info(obs_id, &info);
    if (rc) return rc;
    rk_solve_cfg c{};
    c.n_bstate = info.n_bstate;
    c.interrogate = interrogate;
    const JitKind kinds[] = {JIT_DALTONNG_BOTH, JIT_DALTONNG, JIT_DALTONNG_OBS};
    for (JitKind k : kinds) {
        rc = jit_lookup(jit_key(k, rhs_id, &c, 0, obs_id), nullptr, nullptr);
        if (rc) return rc;
    }
    return RK_OK;
}

int rk_obs_grid_compile_check(int32_t obs_id, int32_t rhs_id, int32_t interrogate) {
    NgObsInfo info;
    int rc = ng_obs_info(obs_id, &info);
    if (rc) return rc;
    rk_solve_cfg c{};
    c.n_bstate = info.n_bstate;
    c.interrogate = interrogate;
    const JitKind kinds[] = {JIT_DALTONNG_GRID_BOTH, JIT_DALTONNG_GRID};
    for (JitKind k : kinds) {
        rc = jit_lookup(jit_key(k, rhs_id, &c, 0, obs_id), nullptr, nullptr);
        if (rc) return rc;
    }
    return RK_OK;
}

int rk_rhs_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate) {
    const UserRhs* u;
    int rc = user_rhs(rhs_id, &u);
    if (rc) return rc;
    rk_solve_cfg c{};
    c.n_bstate = n_bstate;
    c.interrogate = interrogate;
    const bool dense = dense_wanted(*u, n_bstate);
    rc = jit_lookup(jit_key(dense ? JIT_DENSE_ITG : (u->n_bmeas > 1 ? JIT_FWD_M : JIT_FWD), rhs_id, &c), nullptr, nullptr);
    if (rc == RK_OK && !dense && u->n_bmeas > 1) rc = jit_lookup(jit_key(JIT_ITG_M, rhs_id, &c), nullptr, nullptr);     // + the standalone interrogation
    return rc;
}

// The gradient kinds' build for a registered right-hand side, without a device (what rk_rhs_compile_check is for the solver).
// `builtin_too` (Fenrir's two): a built-in id builds the kernel around that right-hand side, which shows without a device that
// fenrir_grad_kernels.hpp is RTC-safe (a built-in one without rhs_generic fails like a source of the solver's kind).
static int grad_compile_check(JitKind kind, bool builtin_too, int32_t rhs_id, int32_t n_bstate, int32_t interrogate) {
    if (!(builtin_too && builtin_rhs_type(rhs_id))) {
        const UserRhs* u;
        const int rc = user_rhs(rhs_id, &u);
        if (rc) return rc;
    }
    rk_solve_cfg c{};
    c.n_bstate = n_bstate;
    c.interrogate = interrogate;
    return jit_lookup(jit_key(kind, rhs_id, &c), nullptr, nullptr);
}

int rk_dalton_grad_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate) {
    return grad_compile_check(JIT_DALTON_GRAD, false, rhs_id, n_bstate, interrogate);
}
int rk_dalton_grad_hyper_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate) {
    return grad_compile_check(JIT_DALTON_GRAD_HYPER, false, rhs_id, n_bstate, interrogate);
}
int rk_fenrir_grad_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate) {
    return grad_compile_check(JIT_FENRIR_GRAD, true, rhs_id, n_bstate, interrogate);
}
int rk_fenrir_grad_hyper_compile_check(int32_t rhs_id, int32_t n_bstate, int32_t interrogate) {
    return grad_compile_check(JIT_FENRIR_GRAD_HYPER, true, rhs_id, n_bstate, interrogate);
}

}  // extern "C"
