// compat/nvbio/strings/alphabet.h -- the alphabets beyond DNA (nvbio/strings/alphabet.h): the 24-letter protein alphabet, 8 bits a
// symbol in a packed vector, and the conversions between symbols and ASCII by alphabet.  The enum, the DNA traits and the DNA
// conversions are basic/dna.h's.
#pragma once
#include "../basic/dna.h"

namespace nvbio {

template <> struct AlphabetTraits<PROTEIN> { static const uint32 SYMBOL_SIZE = 8; static const uint32 SYMBOL_COUNT = 24; };

namespace priv {
/// the protein letters in symbol order; X, the last, stands for everything else
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE const char* protein_letters() { return "ACDEFGHIKLMNOPQRSTVWYBZX"; }
}

NVBIO_FORCEINLINE NVBIO_HOST_DEVICE char protein_to_char(const uint8 c) { return priv::protein_letters()[c < 24u ? c : 23u]; }
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint8 char_to_protein(const char c)
{
    const char* letters = priv::protein_letters();
    for (uint32 k = 0; k < 24u; ++k) if (letters[k] == c) return uint8(k);
    return 23u;
}

template <Alphabet ALPHABET> NVBIO_FORCEINLINE NVBIO_HOST_DEVICE char to_char(const uint8 c)
{
    return ALPHABET == PROTEIN ? protein_to_char(c) : ALPHABET == ASCII ? char(c) : dna_to_char(c);
}
template <Alphabet ALPHABET> NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint8 from_char(const char c)
{
    return ALPHABET == PROTEIN ? char_to_protein(c) : ALPHABET == ASCII ? uint8(c) : char_to_dna(c);
}

/// symbols -> a NUL-terminated string
template <Alphabet ALPHABET, typename SymbolIterator>
NVBIO_HOST_DEVICE inline void to_string(const SymbolIterator begin, const uint32 n, char* string)
{ for (uint32 i = 0; i < n; ++i) string[i] = to_char<ALPHABET>(uint8(begin[i])); string[n] = '\0'; }
template <Alphabet ALPHABET, typename SymbolIterator>
NVBIO_HOST_DEVICE inline void to_string(const SymbolIterator begin, const SymbolIterator end, char* string)
{ uint32 i = 0; for (SymbolIterator it = begin; it != end; ++it) string[i++] = to_char<ALPHABET>(uint8(*it)); string[i] = '\0'; }

/// a [begin, end) range of characters, or a NUL-terminated string, -> symbols
template <Alphabet ALPHABET, typename SymbolIterator>
NVBIO_HOST_DEVICE inline void from_string(const char* begin, const char* end, SymbolIterator symbols)
{ for (uint32 i = 0; begin + i != end; ++i) symbols[i] = from_char<ALPHABET>(begin[i]); }
template <Alphabet ALPHABET, typename SymbolIterator>
NVBIO_HOST_DEVICE inline void from_string(const char* begin, SymbolIterator symbols)
{ for (uint32 i = 0; begin[i] != '\0'; ++i) symbols[i] = from_char<ALPHABET>(begin[i]); }

} // namespace nvbio
