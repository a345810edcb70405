"""Generates scripts/valu_probe10.hip: can `s_setprio` windows make the full-rate ops of two
waves of one SIMD issue together?

probe7 read the G mix as issue slots: a half-rate op (H: v_add3, SDWA xor, v_alignbit) takes
one slot, two adjacent full-rate ops (F: v_add_u32, v_xor_b32) share one, a lone F pays a whole
one.  One wave cannot pair its own F ops (probe9: class order is worth <= 0.3 %), so pairing
would have to come from two waves being inside an F run at the same time.  The arbiter picks
by priority first and age second; this probe raises a wave's priority while it is inside a
run of one class and asks whether the issue rate moves.  The block is probe9's kind 0, the
kernels' G exactly as `make -C spacedrive_amd/csrc asm` lists it (4 columns, class runs of
four: H12 F8 H8 F4 H4 F8 H4 per G), from registers v8..v35.  Arms:
  0  the block unchanged (control)
  1  s_setprio 1 before each F run, s_setprio 0 after it (3 windows per G: F8, F4, F8)
  2  as 1 with priority 3
  3  the inverse: priority 1 over the H runs, 0 over the F runs (the control for "any
     s_setprio changes timing": if 1 and 3 move the rate the same way, it is not pairing)
  4  s_setprio 0 at arm 1's six places (what the instruction itself costs, priority unchanged)
Each arm runs ~1.5 s per reading at 5 waves/SIMD (k_cas_sampled_lanes' occupancy) and at 8
(the earlier probes'; dynamic LDS that nothing touches pins either), twice, the second pass
in rotated order.  Readings: wall-clock T lane-ops/s of the VALU ops (s_setprio not counted)
over the whole reading, lane-ops/clk/CU from the workgroups' s_memtime spans (as probe9
prints it: a workgroup's span is shorter than its launch, so compare it between arms only), the shader clock from s_memtime/s_memrealtime inside
the kernel and from the card's hwmon freq1_input sampled every 20 ms on a host thread while
the arm runs (as power_probe.py reads it).
emit() writes the kernels and the host harness for any list of arms; gen_valu_probe11.py uses it
with its own arms.  With probe11 the harness also samples the board power beside the clock and
prints blocks/s (profiles/g_prio/probe.txt is from before and has neither column).
python scripts/gen_valu_probe10.py  (writes the .hip; build line in its header)"""
import os

from gen_valu_probe9 import H_OPS, schedule

HERE = os.path.dirname(os.path.abspath(__file__))


def runs(lines):
    """[(class, [instructions])] for maximal runs of one class"""
    out = []
    for ln in lines:
        cls = "H" if ln.split()[0] in H_OPS else "F"
        if out and out[-1][0] == cls:
            out[-1][1].append(ln)
        else:
            out.append((cls, [ln]))
    return out


def windows(lines, cls, prio):
    """s_setprio `prio` before each run of class `cls`, s_setprio 0 after it"""
    out = []
    for c, body in runs(lines):
        if c == cls:
            out += [f"s_setprio {prio}"] + body + ["s_setprio 0"]
        else:
            out += body
    return out


def inverse(lines):
    """priority 1 over the H runs.  The block ends in an H run and begins with one, and it
    repeats, so the wave enters the loop at priority 1 (PRE) and each block lowers it before
    an F run and raises it after: six s_setprio per block, as in arm 1."""
    out = []
    for c, body in runs(lines):
        out += (["s_setprio 0"] + body + ["s_setprio 1"]) if c == "F" else body
    return out


G = schedule(4, "rr")
ARMS = [
    # name, block, s_setprio before the loop
    ("control: G x4, the kernels' order", G, 0),
    ("prio 1 over the full-rate runs", windows(G, "F", 1), 0),
    ("prio 3 over the full-rate runs", windows(G, "F", 3), 0),
    ("inverse: prio 1 over the half-rate runs", inverse(G), 1),
    ("s_setprio 0 at arm 1's places", windows(G, "F", 0), 0),
]


def shape(lines, p0):
    """the block as class runs with the priority each runs at, e.g. H12^0 F8^1 H8^0 ..."""
    out, pend = [], []
    prio = p0 if any(ln.startswith("s_setprio") for ln in lines) else None
    for ln in lines:
        if ln.startswith("s_setprio"):
            prio = int(ln.split()[1])
            continue
        cls = "H" if ln.split()[0] in H_OPS else "F"
        if pend and pend[-1][0] == cls and pend[-1][2] == prio:
            pend[-1][1] += 1
        else:
            pend.append([cls, 1, prio])
    for cls, n, p in pend:
        out.append(f"{cls}{n}" + ("" if p is None else f"^{p}"))
    return " ".join(out)


def asm_str(lines):
    return "".join(f'"{ln}\\n"' for ln in lines)


def emit(arms, stem, title, profile, wps=(5, 8)):
    """writes scripts/<stem>.hip: one kernel per arm and the host harness.  An arm is (name,
    block, s_setprio before the loop[, asm input operands that the block names %0, %1, ...]);
    every arm's block has the same number of VALU instructions."""
    arms = [tuple(a) + ("",) * (4 - len(a)) for a in arms]
    body, pre = [], []
    for k, (name, lines, p0, ins) in enumerate(arms):
        body.append(f"    if (ARM == {k}) asm volatile({asm_str(lines)} :: {ins}: CLOB);")
        if p0:
            pre.append(f"    if (ARM == {k}) __builtin_amdgcn_s_setprio({p0});")
    nvalu = len([ln for ln in arms[0][1] if not ln.startswith("s_setprio")])
    assert all(len([ln for ln in l if not ln.startswith("s_setprio")]) == nvalu for _, l, _, _ in arms)
    names = ",\n    ".join(f'{{"{n}", "{shape(l, p0)}"}}' for n, l, p0, _ in arms)
    wps_list = ", ".join(str(w) for w in wps)
    clob = ", ".join(f'"v{i}"' for i in range(8, 36))
    inits = "".join(f"v_mov_b32 v{i}, {i * 2654435761 % 65521}\\n" for i in range(8, 36))
    src = f'''// GENERATED by scripts/gen_{stem}.py -- {title}
// Build: hipcc --offload-arch=gfx950 -O3 -w -pthread -o scripts/{stem} scripts/{stem}.hip
// Run:   scripts/{stem} [seconds per reading, default 1.5] > {profile}
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <dirent.h>
#include <limits.h>
#include <unistd.h>

#define REP 8
#define NVALU {nvalu}  // VALU instructions per asm block (s_setprio not counted)
#define CLOB {clob}
struct Arm {{
    const char* name;
    const char* shape;  // class runs of one block, ^p = the priority the run issues at
}};
static const Arm kArms[] = {{
    {names}}};
constexpr int NARMS = {len(arms)};

template <int ARM>
__global__ __launch_bounds__(256) void k_arm(uint64_t* cyc, uint32_t iters) {{
    asm volatile("{inits}" ::: CLOB);
    __syncthreads();
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
{chr(10).join(pre)}
    for (uint32_t it = 0; it < iters; it++) {{
#pragma unroll
        for (int r = 0; r < REP; r++) {{
{chr(10).join(body)}
        }}
    }}
    __builtin_amdgcn_s_setprio(0);  // every arm leaves at priority 0
    __syncthreads();
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
    uint32_t v;
    asm volatile("v_mov_b32 %0, v8" : "=v"(v));
    if (threadIdx.x == 0) {{  // per-lane (vector) stores of the block's span
        cyc[2 * blockIdx.x] = t1 - t0;
        cyc[2 * blockIdx.x + 1] = (r1 - r0) + (v == 0x12345678u ? 1 : 0);
    }}
}}

template <int K>
struct Table {{
    static void fill(void (**f)(uint64_t*, uint32_t)) {{
        f[K] = k_arm<K>;
        Table<K + 1>::fill(f);
    }}
}};
template <>
struct Table<NARMS> {{
    static void fill(void (**)(uint64_t*, uint32_t)) {{}}
}};

#define HIP_OK(x)                                                                        \\
    do {{                                                                                 \\
        hipError_t e_ = (x);                                                             \\
        if (e_ != hipSuccess) {{                                                          \\
            fprintf(stderr, "%s:%d %s: %s\\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \\
            exit(1);                                                                     \\
        }}                                                                                \\
    }} while (0)

// freq1_input of the visible card's hwmon (matched by PCI address), "" when there is none
static std::string freq_path() {{
    char bus[64] = {{0}};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, 0) != hipSuccess) return "";
    for (char* c = bus; *c; c++) *c = (char)tolower(*c);
    DIR* d = opendir("/sys/class/drm");
    if (!d) return "";
    std::string found;
    while (dirent* e = readdir(d)) {{
        if (strncmp(e->d_name, "card", 4) != 0 || strchr(e->d_name, '-')) continue;
        const std::string dev = std::string("/sys/class/drm/") + e->d_name + "/device";
        char real[PATH_MAX];
        if (!realpath(dev.c_str(), real)) continue;
        const char* base = strrchr(real, '/');
        if (!base || strcmp(base + 1, bus) != 0) continue;
        DIR* h = opendir((dev + "/hwmon").c_str());
        if (!h) continue;
        while (dirent* he = readdir(h)) {{
            if (strncmp(he->d_name, "hwmon", 5) != 0) continue;
            const std::string p = dev + "/hwmon/" + he->d_name + "/freq1_input";
            if (access(p.c_str(), R_OK) == 0) found = p;
        }}
        closedir(h);
    }}
    closedir(d);
    return found;
}}

// power1_average (or power1_input) beside freq1_input, "" when there is none
static std::string power_path(const std::string& fpath) {{
    if (fpath.empty()) return "";
    const std::string dir = fpath.substr(0, fpath.rfind('/') + 1);
    for (const char* n : {{"power1_average", "power1_input"}})
        if (access((dir + n).c_str(), R_OK) == 0) return dir + n;
    return "";
}}

static bool read_ll(const std::string& path, long long* v) {{
    FILE* f = path.empty() ? nullptr : fopen(path.c_str(), "r");
    if (!f) return false;
    const bool ok = fscanf(f, "%lld", v) == 1;
    fclose(f);
    return ok;
}}

static void sample_freq(const std::string& path, const std::string& ppath, const std::atomic<bool>* stop,
                        std::vector<double>* mhz, std::vector<double>* watts) {{
    while (!stop->load()) {{
        long long v = 0;
        if (read_ll(path, &v)) mhz->push_back((double)v / 1e6);
        if (read_ll(ppath, &v)) watts->push_back((double)v / 1e6);  // microwatts
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }}
}}

int main(int argc, char** argv) {{
    const double secs = argc > 1 ? atof(argv[1]) : 1.5;
    hipDeviceProp_t p;
    HIP_OK(hipGetDeviceProperties(&p, 0));
    void (*fns[NARMS])(uint64_t*, uint32_t);
    Table<0>::fill(fns);
    const int cus = p.multiProcessorCount;
    const std::string fpath = freq_path(), ppath = power_path(fpath);
    printf("# %s, %d CUs; each reading loops one arm for %.1f s; T = VALU lane-ops/s by wall clock (HIP events over "
           "the whole reading); lane/clk/CU and cyc/ins from the median workgroup s_memtime span of the last launch; "
           "MHz krn = s_memtime/s_memrealtime in the kernel, MHz hw and W = median hwmon freq1_input and board power over the reading (%s, %s); G blk/s = T / %d, the "
           "blocks of %d VALU ops per lane, in 1e9/s\\n",
           p.gcnArchName, cus, secs, fpath.empty() ? "clock not found" : "sampled every 20 ms",
           ppath.empty() ? "power not found" : "power likewise", NVALU, NVALU);
    for (int k = 0; k < NARMS; k++) {{
        hipFuncAttributes fa;
        HIP_OK(hipFuncGetAttributes(&fa, (const void*)fns[k]));
        printf("# arm %d (%d VGPRs): %s\\n", k, fa.numRegs, kArms[k].shape);
    }}
    printf("# %-4s %-3s %-3s %-42s %9s %8s %12s %8s %8s %7s %6s %9s\\n", "pass", "wps", "arm", "name", "T lane/s",
           "vs arm0", "lane/clk/CU", "cyc/ins", "MHz krn", "MHz hw", "W", "G blk/s");
    const uint32_t iters = (uint32_t)(4096 * 8 / NVALU);
    const double per_wave = (double)iters * REP * NVALU;
    for (int pass = 0; pass < 2; pass++)
        for (int wps : {{{wps_list}}}) {{
            // 256-lane workgroups, one wave per SIMD each; the LDS each asks for (and never touches) lets
            // exactly wps of them share a CU's 160 KiB, so the whole grid is resident at wps waves/SIMD
            const int grid = cus * wps;
            const size_t lds = (size_t)160 * 1024 / wps / 1024 * 1024;
            uint64_t* cyc;
            HIP_OK(hipMalloc(&cyc, (size_t)grid * 16));
            double T[NARMS], lpc[NARMS], cpi[NARMS], mk[NARMS], mh[NARMS], pw[NARMS];
            for (int j = 0; j < NARMS; j++) {{
                const int k = (j + 2 * pass) % NARMS;  // second pass: rotated order
                hipEvent_t e0, e1;
                HIP_OK(hipEventCreate(&e0));
                HIP_OK(hipEventCreate(&e1));
                for (int w = 0; w < 20; w++) hipLaunchKernelGGL(fns[k], dim3(grid), dim3(256), lds, 0, cyc, iters);
                HIP_OK(hipDeviceSynchronize());
                std::vector<double> hz, watts;
                std::atomic<bool> stop(false);
                std::thread th;
                if (!fpath.empty()) th = std::thread(sample_freq, fpath, ppath, &stop, &hz, &watts);
                long launches = 0;
                const auto c0 = std::chrono::steady_clock::now();
                HIP_OK(hipEventRecord(e0));
                do {{
                    for (int r = 0; r < 20; r++) hipLaunchKernelGGL(fns[k], dim3(grid), dim3(256), lds, 0, cyc, iters);
                    launches += 20;
                    HIP_OK(hipStreamSynchronize(0));
                }} while (std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count() < secs);
                HIP_OK(hipEventRecord(e1));
                HIP_OK(hipEventSynchronize(e1));
                stop.store(true);
                if (th.joinable()) th.join();
                float ms = 0;
                HIP_OK(hipEventElapsedTime(&ms, e0, e1));
                std::vector<uint64_t> h((size_t)grid * 2);
                HIP_OK(hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost));
                std::vector<double> c(grid), mhz(grid);
                for (int b = 0; b < grid; b++) {{
                    c[b] = (double)h[2 * b];
                    mhz[b] = (double)h[2 * b] / ((double)h[2 * b + 1] / 100.0);  // s_memrealtime: 100 MHz
                }}
                std::sort(c.begin(), c.end());
                std::sort(mhz.begin(), mhz.end());
                std::sort(hz.begin(), hz.end());
                std::sort(watts.begin(), watts.end());
                T[k] = (double)launches * grid * 256.0 * per_wave / (ms * 1e-3) / 1e12;
                lpc[k] = per_wave * 64.0 * 4 * wps / c[grid / 2];
                cpi[k] = c[grid / 2] / (wps * per_wave);
                mk[k] = mhz[grid / 2];
                mh[k] = hz.empty() ? 0.0 : hz[hz.size() / 2];
                pw[k] = watts.empty() ? 0.0 : watts[watts.size() / 2];
                HIP_OK(hipEventDestroy(e0));
                HIP_OK(hipEventDestroy(e1));
            }}
            for (int k = 0; k < NARMS; k++)
                printf("  %-4d %-3d %-3d %-42s %9.2f %+7.2f%% %12.1f %8.2f %8.0f %7.0f %6.0f %9.1f\\n", pass, wps, k,
                       kArms[k].name, T[k], 100.0 * (T[k] / T[0] - 1.0), lpc[k], cpi[k], mk[k], mh[k], pw[k],
                       T[k] * 1e3 / NVALU);
            fflush(stdout);
            HIP_OK(hipFree(cyc));
        }}
    return 0;
}}
'''
    open(os.path.join(HERE, stem + ".hip"), "w").write(src)


def main():
    emit(ARMS, "valu_probe10", "s_setprio windows over BLAKE3 G's class runs on gfx950", "profiles/g_prio/probe.txt")


if __name__ == "__main__":
    main()
