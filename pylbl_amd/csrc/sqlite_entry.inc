// lbl_absorption(): the compatibility entry with the reference's 11-argument signature
// (pyLBL/c_lib/absorption.c:19-30).  Reads the SQLite file with the same four SELECTs the
// reference issues (absorption.c:69-70; spectral_database.c:55, :113, :143), but only
// once per (path, formula): the line table then stays resident in HBM and later calls are
// one lbl_compute each.
//
// libsqlite3 is bound at run time with dlopen (the image ships the runtime library but
// sqlite3.h only under a conda prefix); the handful of prototypes used are declared here.
#include <dlfcn.h>
#include <sys/stat.h>

#include <cstdlib>
#include <list>
#include <mutex>

namespace {

struct Sqlite
{
    typedef struct sqlite3 sqlite3;
    typedef struct sqlite3_stmt sqlite3_stmt;
    int (*open_v2)(const char *, sqlite3 **, int, const char *) = nullptr;
    int (*close)(sqlite3 *) = nullptr;
    int (*prepare_v2)(sqlite3 *, const char *, int, sqlite3_stmt **, const char **) = nullptr;
    int (*step)(sqlite3_stmt *) = nullptr;
    int (*finalize)(sqlite3_stmt *) = nullptr;
    double (*column_double)(sqlite3_stmt *, int) = nullptr;
    int (*column_int)(sqlite3_stmt *, int) = nullptr;
    const unsigned char * (*column_text)(sqlite3_stmt *, int) = nullptr;
    const char * (*errmsg)(sqlite3 *) = nullptr;
    int (*bind_text)(sqlite3_stmt *, int, const char *, int, void (*)(void *)) = nullptr;
    int (*bind_int)(sqlite3_stmt *, int, int) = nullptr;
    bool ok = false;

    Sqlite()
    {
        const char * names[] = {"libsqlite3.so.0", "libsqlite3.so", "/opt/conda/lib/libsqlite3.so.0"};
        void * lib = nullptr;
        for (const char * name : names)
        {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib != nullptr) break;
        }
        if (lib == nullptr) return;
#define LBL_BIND(field, symbol) \
        field = reinterpret_cast<decltype(field)>(dlsym(lib, symbol)); \
        if (field == nullptr) return;
        LBL_BIND(open_v2, "sqlite3_open_v2")
        LBL_BIND(close, "sqlite3_close")
        LBL_BIND(prepare_v2, "sqlite3_prepare_v2")
        LBL_BIND(step, "sqlite3_step")
        LBL_BIND(finalize, "sqlite3_finalize")
        LBL_BIND(column_double, "sqlite3_column_double")
        LBL_BIND(column_int, "sqlite3_column_int")
        LBL_BIND(column_text, "sqlite3_column_text")
        LBL_BIND(errmsg, "sqlite3_errmsg")
        LBL_BIND(bind_text, "sqlite3_bind_text")
        LBL_BIND(bind_int, "sqlite3_bind_int")
#undef LBL_BIND
        ok = true;
    }
};

const int kSqliteRow = 100, kSqliteDone = 101, kSqliteOpenReadOnly = 1;

struct ResidentMolecule
{
    std::string key;            // path + "\n" + formula
    // What the file looked like when it was read: the reference re-reads the database on every
    // call (absorption.c:44-73), so a file rewritten at the same path must not be served from
    // the copy in HBM.
    long long mtime_ns = 0, size = 0;
    unsigned long long inode = 0;
    int32_t handle = -1;
    bool has_tips = false;
};

struct CompatState
{
    std::mutex mutex;
    lbl_engine * engine = nullptr;
    std::list<ResidentMolecule> resident;       // most recently used first
    size_t limit = 16;                          // LBL_COMPAT_CACHE: molecules kept in HBM
};

// The GPU the compatibility entry computes on: LBL_DEVICE if set, else the launcher's local
// rank (torchrun / Open MPI / Slurm) modulo the number of visible devices, else 0.  Indices
// count the devices HIP shows this process, i.e. they are relative to HIP_VISIBLE_DEVICES.
int compat_device()
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return 0;
    if (const char * text = std::getenv("LBL_DEVICE"))
    {
        char * end = nullptr;
        const long value = std::strtol(text, &end, 10);
        if (end != text && value >= 0) return (int)value;      // out of range: create fails loudly
    }
    for (const char * name : {"LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "SLURM_LOCALID"})
    {
        if (const char * text = std::getenv(name))
        {
            char * end = nullptr;
            const long value = std::strtol(text, &end, 10);
            if (end != text && value >= 0) return (int)(value % count);
        }
    }
    return 0;
}

CompatState & compat_state()
{
    static CompatState state;
    return state;
}

// One molecule's rows as the reference's C reader sees them (absorption.c:44-73): host arrays.
}  // namespace

struct lbl_table
{
    std::string formula;                // molecule.ordinary_formula (the alias asked for if absent)
    int molecule_id = -1;
    std::vector<double> column[7];      // nu, sw, gamma_air, gamma_self, n_air, elower, delta_air
    std::vector<int32_t> local_iso_id;
    std::vector<int64_t> isoid;         // isotopologue rows, in row order
    std::vector<double> iso_mass;
    int num_iso = 0, num_t = 0;         // TIPS: isotopologue-major [num_iso][num_t]
    std::vector<double> tips_t, tips_q;
};

namespace {

Sqlite & sqlite_library()
{
    static Sqlite sql;
    return sql;
}

// Reads `name` from the SQLite file at `path` with the reference's four SELECTs, in the order the
// reference looks things up (alias, partition sums, masses, transitions: absorption.c:50-73), plus
// the molecule's formula.  Returns LBL_OK or the LBL_TABLE_* status of the first thing missing;
// `why` receives the reference's message for it.
int read_table(const char * path, const char * name, lbl_table & out, std::string & why)
{
    Sqlite & sql = sqlite_library();
    if (!sql.ok)
    {
        why = "libsqlite3 could not be loaded.";
        return LBL_ERROR;
    }
    Sqlite::sqlite3 * db = nullptr;
    if (sql.open_v2(path, &db, kSqliteOpenReadOnly, nullptr) != 0 || db == nullptr)
    {
        why = std::string("failed to open ") + path + ".";
        if (db != nullptr) sql.close(db);
        return LBL_TABLE_OPEN_FAILED;
    }
    auto prepare = [&](const char * text, Sqlite::sqlite3_stmt ** stmt) -> bool {
        if (sql.prepare_v2(db, text, -1, stmt, nullptr) != 0)
        {
            why = sql.errmsg(db);
            return false;
        }
        return true;
    };
    int rc = LBL_ERROR;
    Sqlite::sqlite3_stmt * stmt = nullptr;
    int id = -1;
    do
    {
        // spectral_database.c:137-159 (a file without the alias table knows no molecule either)
        if (prepare("select molecule from molecule_alias where alias == ?1", &stmt))
        {
            sql.bind_text(stmt, 1, name, -1, nullptr);
            if (sql.step(stmt) == kSqliteRow) id = sql.column_int(stmt, 0);
            sql.finalize(stmt);
        }
        if (id == -1)
        {
            why = std::string("molecule ") + name + " not found in database.";
            rc = LBL_TABLE_NO_ALIAS;
            break;
        }
        out.molecule_id = id;
        out.formula = name;
        if (prepare("select ordinary_formula from molecule where id == ?1", &stmt))
        {
            sql.bind_int(stmt, 1, id);
            if (sql.step(stmt) == kSqliteRow)
            {
                const unsigned char * text = sql.column_text(stmt, 0);
                if (text != nullptr) out.formula = reinterpret_cast<const char *>(text);
            }
            sql.finalize(stmt);
        }
        // spectral_database.c:49-93
        if (!prepare("select isotopologue_id, temperature, data from tips where molecule_id == ?1",
                     &stmt)) break;
        sql.bind_int(stmt, 1, id);
        int current = -1;
        bool first_row = true;
        while (sql.step(stmt) == kSqliteRow)
        {
            const int which = sql.column_int(stmt, 0);
            if (first_row || which != current) { ++out.num_iso; current = which; first_row = false; }
            out.tips_t.push_back(sql.column_double(stmt, 1));
            out.tips_q.push_back(sql.column_double(stmt, 2));
        }
        sql.finalize(stmt);
        if (out.num_iso == 0)
        {
            why = std::string("no tips data for ") + name + ".";
            rc = LBL_TABLE_NO_TIPS;             // absorption.c:53-59: the reference returns zeros
            break;
        }
        if (out.tips_t.size() % out.num_iso != 0)
        {
            why = "tips data is not rectangular.";      // spectral_database.c:85-90
            rc = LBL_TABLE_NOT_RECTANGULAR;
            break;
        }
        out.num_t = (int)(out.tips_t.size()/out.num_iso);
        // spectral_database.c:108-133
        if (!prepare("select isoid, mass from isotopologue where molecule_id == ?1", &stmt)) break;
        sql.bind_int(stmt, 1, id);
        while (sql.step(stmt) == kSqliteRow)
        {
            out.isoid.push_back(sql.column_int(stmt, 0));
            out.iso_mass.push_back(sql.column_double(stmt, 1));
        }
        sql.finalize(stmt);
        // absorption.c:67-73
        if (!prepare("select nu, sw, gamma_air, gamma_self, n_air, elower, delta_air, "
                     "local_iso_id from transition where molecule_id == ?1", &stmt)) break;
        sql.bind_int(stmt, 1, id);
        while (sql.step(stmt) == kSqliteRow)
        {
            for (int c = 0; c < 7; ++c) out.column[c].push_back(sql.column_double(stmt, c));
            out.local_iso_id.push_back(sql.column_int(stmt, 7));
        }
        sql.finalize(stmt);
        // (everything has been read; what is missing is reported in the order the Python reader
        // of pyLBL's schema looks: isotopologues, then transitions)
        if (out.isoid.empty())
        {
            why = "isotopologues not found for molecule " + std::to_string(id) + ".";
            rc = LBL_TABLE_NO_ISOTOPOLOGUES;
            break;
        }
        if (out.local_iso_id.empty())
        {
            why = "transitions not found for molecule " + std::to_string(id) + ".";
            rc = LBL_TABLE_NO_TRANSITIONS;
            break;
        }
        rc = LBL_OK;
    } while (false);
    sql.close(db);
    return rc;
}

// The table's masses filed under isoid (0 -> 10) like mass_data() does (spectral_database.c:113-129).
bool masses_by_isoid(const lbl_table & table, double mass[lbl::kMassSlots])
{
    std::memset(mass, 0, sizeof(double)*lbl::kMassSlots);
    for (size_t r = 0; r < table.isoid.size(); ++r)
    {
        long long i = table.isoid[r];
        if (i == 0) i = 10;
        if (i < 1 || i >= lbl::kMassSlots) return false;
        mass[i - 1] = table.iso_mass[r];
    }
    return true;
}

int upload_table(lbl_engine * engine, const lbl_table & table, int32_t * molecule)
{
    double mass[lbl::kMassSlots];
    if (!masses_by_isoid(table, mass))
    {
        return fail(engine, LBL_BAD_ARGUMENT, "buffer is too small, increase num_mass.");
    }
    return lbl_molecule_load(
        engine, (int64_t)table.local_iso_id.size(), table.column[0].data(), table.column[1].data(),
        table.column[2].data(), table.column[3].data(), table.column[4].data(),
        table.column[5].data(), table.column[6].data(), table.local_iso_id.data(), mass,
        table.num_iso, table.num_t, table.tips_t.data(), table.tips_q.data(), molecule);
}

// Returns 0 ok, 1 error (message printed), and fills `out`.
int ingest(lbl_engine * engine, const char * path, const char * formula, ResidentMolecule & out)
{
    lbl_table table;
    std::string why;
    const int status = read_table(path, formula, table, why);
    if (status == LBL_TABLE_NO_TIPS)
    {
        out.has_tips = false;       // absorption.c:53-59: rc 0, zeros
        out.handle = -1;
        return 0;
    }
    // (partition sums but no transitions: the reference loops over zero rows and returns zeros
    // with rc 0, absorption.c:76-86; no isotopologue rows: its masses stay unset -- here such rows
    // have no mass, an error once one of them is in range, lbl_molecule_load)
    if (table.local_iso_id.empty() &&
        (status == LBL_TABLE_NO_TRANSITIONS || status == LBL_TABLE_NO_ISOTOPOLOGUES))
    {
        out.has_tips = false;
        out.handle = -1;
        return 0;
    }
    if (status != LBL_OK && status != LBL_TABLE_NO_ISOTOPOLOGUES)
    {
        fprintf(stderr, "Error: %s\n", why.c_str());
        return 1;
    }
    int32_t handle = -1;
    if (upload_table(engine, table, &handle) != LBL_OK)
    {
        fprintf(stderr, "Error: %s\n", lbl_last_error(engine));
        return 1;
    }
    out.handle = handle;
    out.has_tips = true;
    return 0;
}

}  // namespace

extern "C" int lbl_absorption(double pressure, double temperature, double volume_mixing_ratio,
                              int v0, int vn, int n_per_v, double * k, char * database,
                              char * formula, int cut_off, int remove_pedestal)
{
    Sqlite & sql = sqlite_library();
    if (k == nullptr || database == nullptr || formula == nullptr) return 1;
    const long long n = (long long)(vn - v0)*n_per_v;
    if (n > 0) std::memset(k, 0, sizeof(double)*(size_t)n);      // absorption.c:41
    CompatState & state = compat_state();
    std::lock_guard<std::mutex> lock(state.mutex);
    if (!sql.ok)
    {
        fprintf(stderr, "Error: libsqlite3 could not be loaded.\n");
        return 1;
    }
    if (state.engine == nullptr)
    {
        if (lbl_engine_create(compat_device(), &state.engine) != LBL_OK)
        {
            fprintf(stderr, "Error: %s\n", lbl_last_error(nullptr));
            return 1;
        }
        if (const char * text = std::getenv("LBL_COMPAT_CACHE"))
        {
            const long value = std::strtol(text, nullptr, 10);
            if (value >= 1) state.limit = (size_t)value;
        }
    }
    struct stat info;
    if (stat(database, &info) != 0)
    {
        fprintf(stderr, "Error: failed to open %s.\n", database);
        return 1;
    }
    const long long mtime_ns = (long long)info.st_mtim.tv_sec*1000000000ll + info.st_mtim.tv_nsec;
    const std::string key = std::string(database) + "\n" + formula;
    auto found = state.resident.begin();
    for (; found != state.resident.end(); ++found)
    {
        if (found->key == key) break;
    }
    if (found != state.resident.end() &&
        (found->mtime_ns != mtime_ns || found->size != (long long)info.st_size ||
         found->inode != (unsigned long long)info.st_ino))
    {
        // The file changed under the same path: drop the stale copy.
        if (found->handle >= 0) lbl_molecule_free(state.engine, found->handle);
        state.resident.erase(found);
        found = state.resident.end();
    }
    if (found == state.resident.end())
    {
        ResidentMolecule molecule;
        molecule.key = key;
        molecule.mtime_ns = mtime_ns;
        molecule.size = (long long)info.st_size;
        molecule.inode = (unsigned long long)info.st_ino;
        if (ingest(state.engine, database, formula, molecule) != 0) return 1;
        state.resident.push_front(molecule);
        while (state.resident.size() > state.limit)
        {
            // Least recently used goes first.
            if (state.resident.back().handle >= 0)
            {
                lbl_molecule_free(state.engine, state.resident.back().handle);
            }
            state.resident.pop_back();
        }
        found = state.resident.begin();
    }
    else if (found != state.resident.begin())
    {
        state.resident.splice(state.resident.begin(), state.resident, found);
        found = state.resident.begin();
    }
    if (!found->has_tips) return 0;
    const int status = lbl_compute(state.engine, found->handle, 1, &temperature, &pressure,
                                   &volume_mixing_ratio, v0, vn, n_per_v, cut_off,
                                   remove_pedestal, LBL_RANGE_REFERENCE, 0, k, 0, nullptr);
    if (status != LBL_OK)
    {
        fprintf(stderr, "Error: %s\n", lbl_last_error(state.engine));
        return 1;
    }
    return 0;
}

// The reference's own symbol name, so that a build of this library named libabsorption*.so
// can sit behind an unmodified pyLBL/c_lib/gas_optics.py.
extern "C" int absorption(double pressure, double temperature, double volume_mixing_ratio,
                          int v0, int vn, int n_per_v, double * k, char * database,
                          char * formula, int cut_off, int remove_pedestal)
{
    return lbl_absorption(pressure, temperature, volume_mixing_ratio, v0, vn, n_per_v, k, database,
                          formula, cut_off, remove_pedestal);
}

// Inspection of the compatibility entry's state (tests): the device it computes on (-1 before
// the first call) and the number of molecules it holds in HBM.
extern "C" int lbl_compat_state(int32_t * device, int32_t * resident)
{
    CompatState & state = compat_state();
    std::lock_guard<std::mutex> lock(state.mutex);
    if (device != nullptr) *device = state.engine != nullptr ? state.engine->device : -1;
    if (resident != nullptr)
    {
        int count = 0;
        for (const auto & molecule : state.resident) count += molecule.handle >= 0 ? 1 : 0;
        *resident = count;
    }
    return LBL_OK;
}

// ---- The reader by itself (no GPU involved): what Gas.__init__ / database.line_table_of use to get
// a molecule out of the reference's SQLite file at the speed of the C row loop.
extern "C" int lbl_table_read(const char * path, const char * name, lbl_table ** table)
{
    if (path == nullptr || name == nullptr || table == nullptr) return LBL_BAD_ARGUMENT;
    *table = nullptr;
    try
    {
        std::unique_ptr<lbl_table> fresh(new lbl_table());
        std::string why;
        const int status = read_table(path, name, *fresh, why);
        if (status != LBL_OK) return fail(nullptr, status, why);
        *table = fresh.release();
        return LBL_OK;
    }
    catch (const std::exception & e)
    {
        return fail(nullptr, LBL_ERROR, e.what());
    }
}

extern "C" int lbl_table_shape(const lbl_table * table, int64_t * n_lines, int32_t * molecule_id,
                               int32_t * n_isotopologues, int32_t * num_iso, int32_t * num_t,
                               char * formula, int32_t formula_bytes)
{
    if (table == nullptr) return LBL_BAD_ARGUMENT;
    if (n_lines != nullptr) *n_lines = (int64_t)table->local_iso_id.size();
    if (molecule_id != nullptr) *molecule_id = table->molecule_id;
    if (n_isotopologues != nullptr) *n_isotopologues = (int32_t)table->isoid.size();
    if (num_iso != nullptr) *num_iso = table->num_iso;
    if (num_t != nullptr) *num_t = table->num_t;
    if (formula != nullptr && formula_bytes > 0)
    {
        std::snprintf(formula, (size_t)formula_bytes, "%s", table->formula.c_str());
    }
    return LBL_OK;
}

extern "C" int lbl_table_copy(const lbl_table * table, double * columns, int32_t * local_iso_id,
                              int64_t * isoid, double * mass, double * tips_temperature,
                              double * tips_data)
{
    if (table == nullptr) return LBL_BAD_ARGUMENT;
    const size_t n = table->local_iso_id.size();
    if (columns != nullptr)
    {
        for (int c = 0; c < 7; ++c)
        {
            std::memcpy(columns + (size_t)c*n, table->column[c].data(), n*sizeof(double));
        }
    }
    if (local_iso_id != nullptr) std::memcpy(local_iso_id, table->local_iso_id.data(), n*sizeof(int32_t));
    if (isoid != nullptr) std::memcpy(isoid, table->isoid.data(), table->isoid.size()*sizeof(int64_t));
    if (mass != nullptr) std::memcpy(mass, table->iso_mass.data(), table->iso_mass.size()*sizeof(double));
    if (tips_temperature != nullptr)
    {
        std::memcpy(tips_temperature, table->tips_t.data(), (size_t)table->num_t*sizeof(double));
    }
    if (tips_data != nullptr)
    {
        std::memcpy(tips_data, table->tips_q.data(), table->tips_q.size()*sizeof(double));
    }
    return LBL_OK;
}

extern "C" int lbl_table_free(lbl_table * table)
{
    delete table;
    return LBL_OK;
}

// File -> HBM in one call: what lbl_absorption does at the first call on a (path, formula), for
// hosts that hold an engine of their own.
extern "C" int lbl_molecule_load_sqlite(lbl_engine * engine, const char * path, const char * name,
                                        int32_t * molecule)
{
    if (engine == nullptr || path == nullptr || name == nullptr || molecule == nullptr)
    {
        return LBL_BAD_ARGUMENT;
    }
    return entry(engine, [&] {
        lbl_table table;
        std::string why;
        const int status = read_table(path, name, table, why);
        if (status != LBL_OK) return fail(engine, status, why);
        return upload_table(engine, table, molecule);
    });
}
