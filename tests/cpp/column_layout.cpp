// The two column builders of include/dusk_schnorr.hpp (detail::open_columns, detail::keyed_columns) for each of the
// three schemes, over arrays of 3 objects: how many columns, in which order, every base = the address of that field
// in element 0, every stride = sizeof of the struct the field lives in (32 for messages, 4 for idx).  These three
// field lists are all the entry points of the header read their arguments through.  No engine call is made.
// Exit code 0 = all passed; the first mismatch exits with 1.
#include <initializer_list>

#include "dusk_schnorr.hpp"
#include "support.hpp"

using namespace dusk_schnorr;

static void expect(const detail::Columns& got, std::initializer_list<dsv_column> want) {
  CHECK(got.count == (int)want.size());
  int i = 0;
  for (const dsv_column& w : want) {
    CHECK(got.c[i].base == w.base);
    CHECK(got.c[i].stride == w.stride);
    i++;
  }
}

int main() {
  const BlsScalar m[3] = {};
  const uint32_t idx[3] = {0, 1, 2};
  static_assert(sizeof m[0] == 32 && sizeof idx[0] == 4, "the widths dsv.h gives the message and index columns");
  {
    const Signature s[3] = {};
    const PublicKey k[3] = {};
    expect(detail::open_columns(s, k, m), {{&s[0].u_, sizeof s[0]}, {&s[0].R_, sizeof s[0]}, {&k[0].pk, sizeof k[0]}, {m, 32}});
    expect(detail::keyed_columns<PublicKey>(s, idx, m), {{&s[0].u_, sizeof s[0]}, {&s[0].R_, sizeof s[0]}, {idx, 4}, {m, 32}});
    CHECK(detail::open_columns(s, k, m).count == 4 && detail::keyed_columns<PublicKey>(s, idx, m).count == 4);
  }
  {
    const SignatureDouble s[3] = {};
    const PublicKeyDouble k[3] = {};
    expect(detail::open_columns(s, k, m),
           {{&s[0].u_, sizeof s[0]}, {&s[0].R_, sizeof s[0]}, {&s[0].R_prime_, sizeof s[0]},
            {&k[0].pk_, sizeof k[0]}, {&k[0].pk_prime_, sizeof k[0]}, {m, 32}});
    expect(detail::keyed_columns<PublicKeyDouble>(s, idx, m),
           {{&s[0].u_, sizeof s[0]}, {&s[0].R_, sizeof s[0]}, {&s[0].R_prime_, sizeof s[0]}, {idx, 4}, {m, 32}});
    CHECK(detail::open_columns(s, k, m).count == 6 && detail::keyed_columns<PublicKeyDouble>(s, idx, m).count == 5);
  }
  {
    const SignatureVarGen s[3] = {};
    const PublicKeyVarGen k[3] = {};
    expect(detail::open_columns(s, k, m),
           {{&s[0].u_, sizeof s[0]}, {&s[0].R_, sizeof s[0]}, {&k[0].pk_, sizeof k[0]}, {&k[0].generator_, sizeof k[0]}, {m, 32}});
    expect(detail::keyed_columns<PublicKeyVarGen>(s, idx, m), {{&s[0].u_, sizeof s[0]}, {&s[0].R_, sizeof s[0]}, {idx, 4}, {m, 32}});
    CHECK(detail::open_columns(s, k, m).count == 5 && detail::keyed_columns<PublicKeyVarGen>(s, idx, m).count == 4);
  }
  // the strides are the reference's struct sizes, so element 1 of a column is element 1 of the array
  static_assert(sizeof(Signature) == 192 && sizeof(SignatureDouble) == 352 && sizeof(SignatureVarGen) == 192 &&
                    sizeof(PublicKey) == 160 && sizeof(PublicKeyDouble) == 320 && sizeof(PublicKeyVarGen) == 320,
                "the strides above");
  std::printf("ok\n");
  return 0;
}
