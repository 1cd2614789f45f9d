// slim_gate.h -- who may run owner workgroups on a device: the owner gate (a file lock across processes, a mutex inside one) and the
// lease on compute-unit slots.  Host-only C++17: the device's bus id, its compute-unit count and the knobs come in as arguments, so
// g++ builds it and tests/test_slim_gate.py runs it (tests/slim_gate_main.cpp) without a GPU.  Included by slim.hip.
#pragma once

#include "slim_plan.h"

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <string>

namespace mi355rec {
namespace {

// acquire_blocking gave up: another process has held the device's lock for wait_s seconds
struct GateTimeout {
    double wait_s;
};

// Owned rows need a LEASE on compute units.  An owner's steps are static (its row's list), so every owner has to be resident
// together with at least one workgroup that runs the other steps.  That holds for launches whose workgroups all fit the device
// together (one workgroup per compute unit: a row takes most of its LDS) -- and not for persistent kernels that compete for the
// compute units, where the workgroups of each would wait for owners that the others keep out.  The pool below has one slot per
// compute unit; a launch takes what it is allowed (all of them, or MI355REC_SLIM_CUS of them when several models train side by
// side) and sizes its grid by what it got.  A launch that gets fewer than 32 slots runs every step from the in-order queue, which
// makes progress under any residency.
// ... of ONE process: workgroups of another process's persistent kernel are as much in the owners' way as another thread's.  The
// reference's search trains its candidates in a multiprocessing.Pool (ParameterTuning/run_parameter_search.py:498-503): two fits on
// one GPU each used to launch one owner workgroup per compute unit, neither set became resident, and both aborted after the 5 s spin
// budget with S half-updated.  Owners therefore also need the device's OWNER GATE: an advisory file lock (flock, released by the
// kernel when its holder dies) on a per-user, per-device file; the process that holds it runs owners, everybody else runs every
// step from the in-order queue -- slower, never stuck.  Taken with the first lease of a process, given back with the last.
struct OwnerGate {
    std::mutex lock;
    int fd = -1, holders = 0;
    // The device's lock file: per user and per PCI bus id (`bus`), in MI355REC_LOCK_DIR, else XDG_RUNTIME_DIR (a directory only the
    // user can write), else /tmp (SlimKnobs::lock_dir); never through a symbolic link (the name is predictable).  -1: no lock file.
    static int open_lock_file(const SlimKnobs &knobs, std::string bus) {
        for (char &c : bus)
            if (c == ':' || c == '.' || c == '/') c = '_';
        char path[512];
        snprintf(path, sizeof(path), "%s/mi355rec_slim_owners_%u_%s.lock", knobs.lock_dir.c_str(), (unsigned)getuid(), bus.c_str());
        return open(path, O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0600);
    }
    bool acquire(const SlimKnobs &knobs, const std::string &bus) {
        std::lock_guard<std::mutex> g(lock);
        if (holders > 0) { ++holders; return true; }
        if (knobs.no_owner_gate) { ++holders; return true; }
        const int f = open_lock_file(knobs, bus);
        if (f < 0) return false;                       // no lock file, no owners: the queue-only mode is always correct
        if (flock(f, LOCK_EX | LOCK_NB) != 0) {
            close(f);
            return false;                              // another process trains with owners on this device
        }
        fd = f;
        holders = 1;
        return true;
    }
    // Blocking variant for the symmetric store's launch, which has no queue-only mode to fall back to: its long-profile workgroups wait
    // for steps that only its short-profile workgroups run, so TWO such kernels on one device (two handles in threads, two processes)
    // may leave each other's short workgroups non-resident and spin into the 5 s budget.  Symmetric launches of a device
    // therefore run one at a time: `serial` inside the process, the file lock across processes (held from launch to finish).
    // The file lock is polled (LOCK_NB) OUTSIDE the gate's mutex against a deadline (MI355REC_SLIM_GATE_WAIT_S, default 600 s): a
    // process that hangs with the lock held makes this launch fail with a message (GateTimeout, with `serial` unlocked again), not
    // block for ever -- and never blocks the acquire / release of the dense store's launches of this process.
    std::mutex serial;
    bool acquire_blocking(const SlimKnobs &knobs, const std::string &bus) {
        serial.lock();
        {
            std::lock_guard<std::mutex> g(lock);
            if (holders > 0 || knobs.no_owner_gate) { ++holders; return true; }
        }
        const int f = open_lock_file(knobs, bus);
        bool locked = false;
        if (f >= 0) {
            const double wait_s = knobs.gate_wait_s;
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(wait_s);
            for (;;) {
                if (flock(f, LOCK_EX | LOCK_NB) == 0) { locked = true; break; }
                if (errno != EWOULDBLOCK && errno != EINTR) break;          // (no usable lock file: in-process serialisation only)
                if (std::chrono::steady_clock::now() >= deadline) {
                    close(f);
                    serial.unlock();
                    throw GateTimeout{wait_s};
                }
                usleep(2000);
            }
            if (!locked) close(f);
        }
        std::lock_guard<std::mutex> g(lock);
        if (holders > 0) {                                 // (a dense launch of this process took the gate meanwhile: its lock serves)
            if (locked) { (void)flock(f, LOCK_UN); close(f); }
            ++holders;
            return true;
        }
        if (locked) fd = f;
        holders = 1;
        return true;
    }
    void release_blocking() {
        release();
        serial.unlock();
    }
    void release() {
        std::lock_guard<std::mutex> g(lock);
        if (holders > 0 && --holders == 0 && fd >= 0) {
            (void)flock(fd, LOCK_UN);
            close(fd);
            fd = -1;
        }
    }
};
inline OwnerGate &owner_gate() {
    static OwnerGate *g = new OwnerGate();
    return *g;
}

// free compute-unit slots of the process (-1: not counted yet)
inline std::atomic<int> &owner_slots() {
    static std::atomic<int> slots{-1};
    return slots;
}
struct OwnerLease {
    int slots = 0;
    bool gated = false;
    void take(bool wanted, int want, int cus, const SlimKnobs &knobs, const std::string &bus) {
        if (!wanted) return;
        if (!owner_gate().acquire(knobs, bus)) return;           // (slots stays 0: queue-only launch)
        gated = true;
        int expected = -1;
        owner_slots().compare_exchange_strong(expected, cus);      // first use: one slot per compute unit
        int have = owner_slots().load();
        while (have >= 32) {
            const int n = std::min(have, want);
            if (owner_slots().compare_exchange_weak(have, have - n)) { slots = n; return; }
        }
    }
    void give_back() {
        if (slots) owner_slots().fetch_add(slots);
        slots = 0;
        if (gated) owner_gate().release();
        gated = false;
    }
    ~OwnerLease() { give_back(); }
};

}  // namespace
}  // namespace mi355rec
