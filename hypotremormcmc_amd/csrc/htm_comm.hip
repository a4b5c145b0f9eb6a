// htm_comm.hip -- RCCL reached from the C ABI (include/htm_hip.h: htm_comm_*, htm_chains_run_lockstep_comm), so that a
// Fortran / C host needs no Python to use RCCL for the swap.  librccl is bound at run time (dlopen): the library itself does
// not link against it, and inside a PyTorch process the copy torch has already loaded is reused.  Only the four entry points
// the swap needs.  Of a chain set this unit reads its ranks, its device and the length of its swap record.
#include "htm_host.hpp"

#include <dlfcn.h>

using namespace htm;

extern "C" {

struct htm_comm {
    void *lib = nullptr, *comm = nullptr;
    int rank = 0, n_ranks = 1, device = 0;
    int (*all_gather)(const void *, void *, size_t, int, void *, void *) = nullptr;
    int (*comm_destroy)(void *) = nullptr;
    double *d_gathered = nullptr;
    size_t gathered_cap = 0;
};
namespace {
struct NcclId { char b[HTM_COMM_ID_BYTES]; };
void *rccl_open()
{
    static void *lib = [] {
        const char *names[] = {getenv("HTM_RCCL_LIB"), "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        void *h = nullptr;
        for (const char *n : names) {
            if (!n || !*n) continue;
            if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD))) break;      // already in the process (PyTorch's copy)
        }
        for (const char *n : names) {
            if (h) break;
            if (!n || !*n) continue;
            h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        }
        return h;
    }();
    return lib;
}
}  // namespace

int htm_comm_unique_id(void *id, size_t id_bytes)
{
    if (!id || id_bytes < HTM_COMM_ID_BYTES) return fail(HTM_EINVAL, "id buffer must hold %d bytes", HTM_COMM_ID_BYTES);
    void *lib = rccl_open();
    if (!lib) return fail(HTM_ENODEVICE, "librccl.so not found (%s)", dlerror());
    auto get_id = reinterpret_cast<int (*)(NcclId *)>(dlsym(lib, "ncclGetUniqueId"));
    if (!get_id) return fail(HTM_ENODEVICE, "ncclGetUniqueId not found in librccl");
    NcclId u;
    std::memset(&u, 0, sizeof(u));
    const int st = get_id(&u);
    if (st != 0) return fail(HTM_EHIP, "ncclGetUniqueId failed with status %d", st);
    std::memset(id, 0, id_bytes);
    std::memcpy(id, &u, sizeof(u));
    return HTM_OK;
}

int htm_comm_create(const void *id, size_t id_bytes, int rank, int n_ranks, int device, htm_comm **out)
{
    if (!out) return fail(HTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (!id || id_bytes < HTM_COMM_ID_BYTES || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(HTM_EINVAL, "bad argument");
    int rc = use_device(device);
    if (rc) return rc;
    void *lib = rccl_open();
    if (!lib) return fail(HTM_ENODEVICE, "librccl.so not found (%s)", dlerror());
    auto init_rank = reinterpret_cast<int (*)(void **, int, NcclId, int)>(dlsym(lib, "ncclCommInitRank"));
    auto all_gather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, void *)>(dlsym(lib, "ncclAllGather"));
    auto destroy = reinterpret_cast<int (*)(void *)>(dlsym(lib, "ncclCommDestroy"));
    if (!init_rank || !all_gather || !destroy) return fail(HTM_ENODEVICE, "librccl lacks ncclCommInitRank / ncclAllGather / ncclCommDestroy");
    NcclId u;
    std::memcpy(&u, id, sizeof(u));
    void *comm = nullptr;
    const int st = init_rank(&comm, n_ranks, u, rank);
    if (st != 0 || !comm) return fail(HTM_EHIP, "ncclCommInitRank failed with status %d (RCCL refuses two ranks on one device)", st);
    htm_comm *c = new htm_comm();
    c->lib = lib; c->comm = comm; c->rank = rank; c->n_ranks = n_ranks; c->device = device;
    c->all_gather = all_gather; c->comm_destroy = destroy;
    *out = c;
    return HTM_OK;
}

int htm_comm_destroy(htm_comm *c)
{
    if (!c) return HTM_OK;
    (void)hipSetDevice(c->device);
    if (c->d_gathered) (void)hipFree(c->d_gathered);
    if (c->comm && c->comm_destroy) (void)c->comm_destroy(c->comm);
    delete c;
    return HTM_OK;
}

int htm_comm_allgather(htm_comm *c, const void *d_send, void *d_recv, size_t bytes_per_rank, void *hip_stream)
{
    if (!c || !d_send || !d_recv) return fail(HTM_EINVAL, "NULL argument");
    const int st = c->all_gather(d_send, d_recv, bytes_per_rank, 0 /* ncclInt8 */, c->comm, hip_stream);
    if (st != 0) return fail(HTM_EHIP, "ncclAllGather failed with status %d", st);
    return HTM_OK;
}

int htm_chains_run_lockstep_comm(htm_chains *hc, int n_iter, htm_comm *c)
{
    if (!hc || !c) return fail(HTM_EINVAL, "NULL argument");
    if (c->n_ranks != hc->dev.n_procs || c->rank != hc->dev.rank) return fail(HTM_EINVAL, "communicator rank/size do not match the chain set");
    HIPCHK(hipSetDevice(hc->fwd->device));
    const size_t words = swap_words(hc->dev.n_chains) * (size_t)c->n_ranks;
    if (words > c->gathered_cap) {
        if (c->d_gathered) HIPCHK(hipFree(c->d_gathered));
        c->d_gathered = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&c->d_gathered), words * sizeof(double)));
        c->gathered_cap = words;
    }
    return htm_chains_run_lockstep(hc, n_iter, c->all_gather, c->comm, c->d_gathered);
}

}  // extern "C"
