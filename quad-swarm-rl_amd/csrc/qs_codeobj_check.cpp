// qs_codeobj_check.cpp - the code-object checker (docs/UPSTREAM_SPILL_BUG.md): disassembles a code object, scans the block
// prologues for a VGPR spill / copy in front of an exec restore and, where it is provably safe, moves the restore.  Host code only.
#include "qs_codeobj_check.h"

#include <cctype>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <spawn.h>
#include <sstream>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

extern char **environ;

namespace qs_check {

bool read_file(const std::string &path, std::string &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[65536]; size_t n;
    out.clear();
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
bool file_exists(const std::string &path) { struct stat st; return stat(path.c_str(), &st) == 0 && st.st_size > 0; }

void split_words(const std::string &flags, std::vector<std::string> &argv) {
    std::istringstream in(flags);
    for (std::string word; in >> word;) argv.push_back(word);
}
int run_program(const std::vector<std::string> &argv, const std::string &log, const std::function<void(FILE *)> &read_stdout) {
    std::vector<char *> av;
    for (const std::string &a : argv) av.push_back(const_cast<char *>(a.c_str()));
    av.push_back(nullptr);
    int fds[2] = {-1, -1};
    if (read_stdout && pipe2(fds, O_CLOEXEC) != 0) return -1;   // (the child's copy on fd 1 stays open across its exec)
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_addopen(&fa, 2, log.empty() ? "/dev/null" : log.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    posix_spawn_file_actions_adddup2(&fa, read_stdout ? fds[1] : 2, 1);
    pid_t pid = -1;
    const bool started = posix_spawnp(&pid, av[0], &fa, nullptr, av.data(), environ) == 0;
    posix_spawn_file_actions_destroy(&fa);
    if (read_stdout) {
        close(fds[1]);
        FILE *f = started ? fdopen(fds[0], "r") : nullptr;
        if (f) { read_stdout(f); fclose(f); } else close(fds[0]);
    }
    int st = 0;
    if (!started || waitpid(pid, &st, 0) != pid) return -1;
    return WIFEXITED(st) ? WEXITSTATUS(st) : -1;
}

// ---- code-object verification ------------------------------------------------------------------------------------------
// ROCm 7.2's register allocator can place a VGPR spill, reload, copy or rematerialised constant at the top of a control-flow JOIN block in
// front of the instruction that restores exec there (`s_or_b64 exec, exec, s[a:b]`): the scalar allocator, which runs first, puts its own
// spills / copies at the very top of the block (they do not depend on exec), and the vector allocator's "skip the block prologue" stops at
// the first of those that is not a spill.  A wave that reaches the join through the branch that skipped the `then` side arrives with
// exec == 0: the spill stores nothing and the later reload returns stale scratch memory.  That is what round 5's unexplained parity
// failure was (single-wave N = 17 object with the RP-tracker flag: the environment index came back as a float, the counter loads faulted),
// and the default objects only differed from it by luck: 18 of 269 cached objects carried the pattern somewhere.  Every specialised object
// is therefore disassembled and scanned before it is used; an object with the pattern is rebuilt with other scheduler settings (instruction
// order and register assignment change, results do not) and, if none is clean, not used at all (generic kernels, loudly).
static std::string llvm_bin() { const char *ev = getenv("QS_LLVM_BIN"); return (ev && ev[0]) ? ev : "/opt/rocm/lib/llvm/bin"; }
static bool starts_with(const std::string &t, const char *p) { return t.compare(0, strlen(p), p) == 0; }
// instructions of a block prologue that do not depend on exec (SGPR spills to VGPR lanes, scalar moves / adds, waits)
static bool hz_silent(const std::string &t) {
    static const char *const k[] = {"v_writelane_b32", "v_readlane_b32", "s_nop", "s_waitcnt", "s_mov_b32", "s_mov_b64", "s_add_i32",
        "s_add_u32", "s_addk_i32"};
    for (const char *q : k) if (starts_with(t, q)) return t.find("exec") == std::string::npos;
    return false;
}
// ... and those that do: what the vector register allocator inserts (spill, reload, copy, rematerialised constant, AGPR copy)
static bool hz_exec_dependent(const std::string &t) {
    return starts_with(t, "scratch_load_") || starts_with(t, "scratch_store_") || starts_with(t, "v_mov_b32")
        || starts_with(t, "v_mov_b64") || starts_with(t, "v_accvgpr_");
}
// the exec restore of a join / else block: s_or_b64 exec, exec, s[..] | s_xor_b64 exec, exec, s[..] | s_or_saveexec_b64 s[..], s[..]  (NOT
// `, -1`: whole-wave mode)
static bool hz_restore(const std::string &t) {
    if (starts_with(t, "s_or_b64 exec, exec, s[") || starts_with(t, "s_xor_b64 exec, exec, s[")) return true;
    return starts_with(t, "s_or_saveexec_b64 s[") && t.find("], s[") != std::string::npos;
}
// One hazard: the block prologue (instructions + encodings) in front of a misplaced exec restore, the restore itself, what follows it.
struct SpecHazard { std::string kernel, label; std::vector<std::string> ins, raw; std::string restore, restore_raw;
    std::vector<std::string> after; };
static std::string hz_describe(const SpecHazard &h) {
    std::string o = h.kernel + " <" + h.label + ">:";
    for (const std::string &t : h.ins) o += " " + t + " ;";
    return o + " " + h.restore;
}
// Scan `llvm-objdump -d --symbolize-operands` text (instruction, then `// address: encoding dwords`).
static void spec_scan_disassembly(FILE *f, std::vector<SpecHazard> &out) {
    char line[1024];
    std::string kernel = "?";
    SpecHazard cur;
    bool scanning = false, dependent = false;
    int follow = 0;   // instructions still to record behind the last hazard's restore
    while (fgets(line, sizeof line, f)) {
        std::string t(line);
        while (!t.empty() && (t.back() == '\n' || t.back() == '\r' || t.back() == ' ' || t.back() == '\t')) t.pop_back();
        const size_t lt = t.find(" <"), gt = t.rfind(">:");
        if (!t.empty() && isxdigit((unsigned char)t[0]) && lt != std::string::npos && gt == t.size() - 2) {   // "0000000000002b60 <L14>:"
            const std::string label = t.substr(lt + 2, gt - lt - 2);
            if (!(label.size() > 1 && label[0] == 'L' && isdigit((unsigned char)label[1]))) kernel = label;
            cur = SpecHazard(); cur.kernel = kernel; cur.label = label;
            scanning = true; dependent = false; follow = 0;
            continue;
        }
        const size_t cm = t.find("//");
        if (cm == std::string::npos) continue;
        std::string raw;   // the encoding as bytes (little-endian dwords)
        {
            const size_t colon = t.find(':', cm);
            if (colon != std::string::npos) {
                const char *q = t.c_str() + colon + 1;
                while (*q) {
                    while (*q == ' ') ++q;
                    if (!isxdigit((unsigned char)*q)) break;
                    char *e = nullptr;
                    const unsigned long w = strtoul(q, &e, 16);
                    if (e - q != 8) break;
                    for (int b = 0; b < 4; ++b) raw.push_back((char)((w >> (8 * b)) & 0xff));
                    q = e;
                }
            }
        }
        t.resize(cm);
        size_t b = 0;
        while (b < t.size() && (t[b] == ' ' || t[b] == '\t')) ++b;
        t = t.substr(b);
        while (!t.empty() && (t.back() == ' ' || t.back() == '\t')) t.pop_back();
        if (t.empty()) continue;
        if (follow > 0) { out.back().after.push_back(t); --follow; }
        if (!scanning) continue;
        if (hz_restore(t)) {
            if (dependent) { cur.restore = t; cur.restore_raw = raw; out.push_back(cur); follow = 6; }
            scanning = false;
        } else if (hz_exec_dependent(t)) { dependent = true; cur.ins.push_back(t); cur.raw.push_back(raw); }
        else if (hz_silent(t)) { cur.ins.push_back(t); cur.raw.push_back(raw); }
        else scanning = false;
    }
}
// the plain gfx950 code objects inside `path` - a bundle (hipcc --genco), a plain object, or a shared library whose .hip_fatbin section
// holds one bundle per translation unit - written to temporary files (the caller unlinks them)
static int spec_extract_elfs(const std::string &path, std::vector<std::string> &elfs, std::string &why) {
    static int serial = 0;
    char tag[96];
    snprintf(tag, sizeof tag, "/tmp/qs_verify_%ld_%d", (long)getpid(), serial++);
    const std::string base = tag, bin = llvm_bin();
    std::string blob;
    if (path.size() > 3 && path.compare(path.size() - 3, 3, ".so") == 0) {
        const std::string fat = base + ".fatbin";
        const int rc = run_program({bin + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path, base + ".copy"}, "");
        unlink((base + ".copy").c_str());
        const bool ok = rc == 0 && read_file(fat, blob);
        unlink(fat.c_str());
        if (!ok) { why = "cannot extract .hip_fatbin from " + path + " (QS_LLVM_BIN=" + bin + ")"; return -1; }
    } else if (!read_file(path, blob)) { why = "cannot read " + path; return -1; }
    const std::string magic = "__CLANG_OFFLOAD_BUNDLE__";
    int k = 0;
    for (size_t at = blob.find(magic); at != std::string::npos; ++k) {
        const size_t next = blob.find(magic, at + magic.size());
        const std::string part = base + "." + std::to_string(k) + ".bundle", elf = base + "." + std::to_string(k) + ".elf";
        FILE *f = fopen(part.c_str(), "wb");
        if (!f) { why = "cannot write " + part; return -1; }
        fwrite(blob.data() + at, 1, (next == std::string::npos ? blob.size() : next) - at, f);
        fclose(f);
        const bool ok = run_program({bin + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
            "--input=" + part, "--output=" + elf}, "") == 0 && file_exists(elf);
        unlink(part.c_str());
        if (ok) elfs.push_back(elf); else unlink(elf.c_str());
        at = next;
    }
    if (k == 0) {   // not a bundle: a plain code object (copied, so that the caller can unlink uniformly)
        const std::string elf = base + ".plain.elf";
        FILE *f = fopen(elf.c_str(), "wb");
        if (!f) { why = "cannot write " + elf; return -1; }
        fwrite(blob.data(), 1, blob.size(), f);
        fclose(f);
        elfs.push_back(elf);
    }
    if (elfs.empty()) { why = "no gfx950 code object in " + path; return -1; }
    return 0;
}
static int spec_find_hazards(const std::string &path, std::vector<SpecHazard> &hz, std::string &why) {
    std::vector<std::string> elfs;
    if (spec_extract_elfs(path, elfs, why) != 0) { for (const std::string &e : elfs) unlink(e.c_str()); return -1; }
    int rc = 0;
    for (const std::string &elf : elfs) {
        if (rc == 0 && run_program({llvm_bin() + "/llvm-objdump", "-d", "--symbolize-operands", elf}, "",
                [&](FILE *f) { spec_scan_disassembly(f, hz); }) != 0) {
            rc = -1; why = "llvm-objdump failed on " + path + " (QS_LLVM_BIN=" + llvm_bin() + ")"; }
        unlink(elf.c_str());
    }
    return rc;
}
// 0 = clean, 1 = the pattern is there (report: one line per place), < 0 = could not be checked (tools missing, not a code object)
int spec_verify_file(const std::string &path, std::string &report) {
    std::vector<SpecHazard> hz;
    if (spec_find_hazards(path, hz, report) != 0) return -1;
    for (const SpecHazard &h : hz) report += hz_describe(h) + "\n";
    return hz.empty() ? 0 : 1;
}
// scalar registers named in an operand text: "s5" -> {5}, "s[4:7]" -> {4..7}
static void hz_sregs(const std::string &t, std::vector<int> &regs) {
    for (size_t k = 0; k < t.size(); ++k) {
        if (t[k] != 's' || (k > 0 && (isalnum((unsigned char)t[k - 1]) || t[k - 1] == '_'))) continue;
        if (k + 1 < t.size() && t[k + 1] == '[') {
            int lo = 0, hi = 0;
            if (sscanf(t.c_str() + k, "s[%d:%d]", &lo, &hi) == 2) for (int r = lo; r <= hi; ++r) regs.push_back(r);
        } else if (k + 1 < t.size() && isdigit((unsigned char)t[k + 1])) regs.push_back(atoi(t.c_str() + k + 1));
    }
}
// REPAIR: the exec restore moves to the front of its block prologue (as far forward as the definition of the mask it reads allows) -
// straight-line code that nobody jumps into; every other instruction keeps its place relative to the others.  Made only where it provably
// changes nothing else:
//   * no exec-dependent instruction sits in front of a prologue instruction that writes the SGPR pair the restore reads;
// * none of the last five prologue instructions is a v_readlane (VALU-writes-SGPR -> VMEM-reads-it needs 5 wait states, and the restore was
//     one of them); the first two instructions behind the restore are neither DPP nor lane operations (VALU-write -> DPP wait states);
//   * the byte sequence occurs in the file exactly as often as the scan reports it.
// Returns the number of places repaired (file rewritten in place), `left` = the ones that were not, with the reason; < 0 on errors.
int spec_repair_file(const std::string &path, std::string &left) {
    std::vector<SpecHazard> hz;
    std::string why;
    if (spec_find_hazards(path, hz, why) != 0) { left = why; return -1; }
    if (hz.empty()) return 0;
    std::string blob;
    if (!read_file(path, blob)) { left = "cannot read " + path; return -1; }
    int repaired = 0;
    std::vector<bool> done(hz.size(), false);
    for (size_t a = 0; a < hz.size(); ++a) {
        if (done[a]) continue;
        const SpecHazard &h = hz[a];
        std::string old_bytes;
        for (const std::string &r : h.raw) old_bytes += r;
        old_bytes += h.restore_raw;
        int same = 0;   // hazards with the identical byte sequence (the same code in two kernels)
        for (size_t b = a; b < hz.size(); ++b) {
            std::string ob;
            for (const std::string &r : hz[b].raw) ob += r;
            ob += hz[b].restore_raw;
            if (ob == old_bytes) { done[b] = true; ++same; }
        }
        // what the restore reads (and, for s_or_saveexec, also writes)
        std::vector<int> need;
        const size_t c1 = h.restore.find(',');
        hz_sregs(starts_with(h.restore, "s_or_saveexec")
            ? h.restore.substr(h.restore.find(' ')) : h.restore.substr(h.restore.find(',', c1 + 1)), need);
        size_t pos = 0;
        for (size_t k = 0; k < h.ins.size(); ++k) {
            const std::string &t = h.ins[k];
            if (!hz_silent(t) || starts_with(t, "s_nop") || starts_with(t, "s_waitcnt") || starts_with(t, "v_writelane")) continue;
            std::vector<int> wr;
            const size_t sp = t.find(' ');
            hz_sregs(t.substr(sp == std::string::npos ? 0 : sp, t.find(',') == std::string::npos ? std::string::npos : t.find(',') - sp),
                wr);
            for (int w : wr) for (int n : need) if (w == n) pos = k + 1;
        }
        std::string reason;
        for (size_t k = 0; k < pos; ++k) if (hz_exec_dependent(h.ins[k])) reason = "an exec-dependent instruction sits in front of the definition of the saved mask";
        // VALU writes an SGPR (v_readlane) -> a VMEM instruction / a lane select reads it: 5 wait states, and the restore was one of them
        for (size_t k = h.ins.size() >= 5 ? h.ins.size() - 5 : 0; k < h.ins.size(); ++k) {
            if (!starts_with(h.ins[k], "v_readlane")) continue;
            std::vector<int> wr;
            hz_sregs(h.ins[k].substr(0, h.ins[k].find(',')), wr);
            for (size_t a2 = 0; a2 < h.after.size() && a2 < 5; ++a2) {
                const std::string &u = h.after[a2];
                const bool vmem = starts_with(u, "buffer_") || starts_with(u, "global_") || starts_with(u, "flat_")
                    || starts_with(u, "scratch_") || starts_with(u, "v_readlane") || starts_with(u, "v_writelane");
                if (!vmem) continue;
                std::vector<int> rd;
                hz_sregs(u, rd);
                for (int w : wr) for (int r : rd) if (w == r) reason = "a v_readlane near the end of the prologue feeds a memory / lane instruction right behind the restore";
            }
        }
        for (size_t k = 0; k < h.after.size() && k < 2; ++k)
            if (h.after[k].find("dpp") != std::string::npos || starts_with(h.after[k], "v_readlane")
                || starts_with(h.after[k], "v_writelane")
                || starts_with(h.after[k], "v_readfirstlane")) reason = "DPP / lane operation right behind the restore";
        if (h.restore_raw.empty() || old_bytes.size() < 8) reason = "no encoding in the disassembly";
        if (reason.empty()) {
            size_t count = 0;
            for (size_t at = blob.find(old_bytes); at != std::string::npos; at = blob.find(old_bytes, at + 1)) ++count;
            if ((int)count != same) reason = "byte sequence found " + std::to_string(count) + " times in the file, " + std::to_string(same) + " expected";
        }
        if (!reason.empty()) { left += hz_describe(h) + "   [" + reason + "]\n"; continue; }
        std::string new_bytes;
        for (size_t k = 0; k < pos; ++k) new_bytes += h.raw[k];
        new_bytes += h.restore_raw;
        for (size_t k = pos; k < h.ins.size(); ++k) new_bytes += h.raw[k];
        for (size_t at = blob.find(old_bytes); at != std::string::npos;
            at = blob.find(old_bytes, at + new_bytes.size())) blob.replace(at, old_bytes.size(), new_bytes);
        repaired += same;
    }
    if (repaired > 0) {
        struct stat st;
        const std::string tmp = path + ".repair.tmp";
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f) { left = "cannot write " + tmp; return -1; }
        fwrite(blob.data(), 1, blob.size(), f);
        fclose(f);
        if (stat(path.c_str(), &st) == 0) chmod(tmp.c_str(), st.st_mode);
        if (rename(tmp.c_str(), path.c_str()) != 0) { unlink(tmp.c_str()); left = "cannot replace " + path; return -1; }
    }
    return repaired;
}
Checked spec_check_file(const std::string &path) {
    Checked c;
    c.status = spec_verify_file(path, c.report);
    if (c.status != 1) return c;
    c.moved = spec_repair_file(path, c.left);
    if (c.moved > 0) { c.report.clear(); c.status = spec_verify_file(path, c.report); }
    return c;
}

}   // namespace qs_check

#ifdef QS_CHECK_MAIN
// qs_spec_check verify|repair|clean PATH...   (a directory = every .hsaco / .so in it; clean = verify, repair if needed, verify again)
// stdout: the report / the places left, as qs_spec_verify / qs_spec_repair return them; stderr: one line per file, and a total for several.
// Exit status: 0 = clean, 1 = the pattern is present, 2 = could not be checked.
#include <algorithm>
#include <dirent.h>
int main(int argc, char **argv) {
    using namespace qs_check;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (argc < 3 || (cmd != "verify" && cmd != "repair" && cmd != "clean")) {
        fprintf(stderr, "usage: %s verify|repair|clean PATH...\n", argv[0]);
        return 2;
    }
    std::vector<std::string> paths;
    for (int a = 2; a < argc; ++a) {
        DIR *d = opendir(argv[a]);
        if (!d) { paths.push_back(argv[a]); continue; }
        std::vector<std::string> found;
        while (const dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if ((n.size() > 6 && n.compare(n.size() - 6, 6, ".hsaco") == 0) || (n.size() > 3 && n.compare(n.size() - 3, 3, ".so") == 0))
                found.push_back(std::string(argv[a]) + "/" + n);
        }
        closedir(d);
        std::sort(found.begin(), found.end());
        paths.insert(paths.end(), found.begin(), found.end());
    }
    int flagged = 0, worst = 0;
    for (const std::string &p : paths) {
        Checked c;
        if (cmd == "verify") c.status = spec_verify_file(p, c.report);
        else if (cmd == "clean") c = spec_check_file(p);
        else { c.moved = spec_repair_file(p, c.left); c.status = c.moved < 0 ? -1 : (c.left.empty() ? 0 : 1); }
        const std::string text = c.report + c.left;
        fputs(text.c_str(), stdout);
        if (!text.empty() && text.back() != '\n') fputc('\n', stdout);   // (the reason a file could not be checked has no line end)
        fflush(stdout);
        const std::string moved = c.moved > 0 ? "  (" + std::to_string(c.moved) + " exec restore(s) moved)" : "";
        fprintf(stderr, "%s %s%s\n", p.substr(p.rfind('/') + 1).c_str(), c.status == 0 ? "clean" : (c.status == 1 ? "HAZARD" : "NOT CHECKED"),
            moved.c_str());
        flagged += c.status == 1;
        worst = std::max(worst, c.status < 0 ? 2 : c.status);
    }
    if (paths.size() > 1) fprintf(stderr, "%zu files, %d with a VGPR spill / copy in front of an exec restore\n", paths.size(), flagged);
    return worst;
}
#endif
